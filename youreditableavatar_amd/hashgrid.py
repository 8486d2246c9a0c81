"""The geometry stage's SDF field: the multiresolution hash-grid encoding and the fused field built on it, with gradients.

``HashGrid(n_input_dims, config)`` has the call shape of ``tcnn.Encoding`` for what the reference's ``TCNNEncoding`` and ``ProgressiveBandHashGrid``
(``tetgs_spatial/models/networks.py`` :55-95) build; ``SdfField(encoding, mlp)`` is ``forward_sdf`` of ``models/geometry/implicit_sdf.py``: the box map of
``contract_to_unisphere`` (``unbounded=False``), the encoding, the bias-free ``VanillaMLP`` (:151-188) and ``sdf_bias``, in one kernel that stores nothing of
size N x 32 or N x 64.  The kernels are ``csrc/tgs_hashgrid.hip``; the rules are written down in include/tgs_raster.h, "hash-grid field", and restated in
tests/hashgrid_ref.py.  HIP device only: there is no CPU path (``level_table`` alone is pure Python and numpy).  float32 only.

The parameter layout (level-major, then entry, then feature) is the published layout of tiny-cuda-nn's grid encoding, so a float32 ``encoding.params``
tensor of a checkpoint loads as it is -- nobody could check that against tiny-cuda-nn itself, which is not installed where this project runs; the rules of
the header are what the tests pin.  ``levels=`` takes an explicit table for a checkpoint whose producer rounded a level's scale otherwise.

Not served: ``normal_type="analytic"`` (it needs a double backward, which raises here; the finite-difference normals are three more field calls),
feature outputs on the fused path (``n_feature_dims > 0``: 1 to 4 outputs of ONE network are served), tcnn's other encodings and its networks, other
feature counts than 2, ``interpolation`` other than ``"Linear"``, dense and tiled grids, half precision.  There are no float atomics: two runs give the same
bits, forward and backward.  At most 2^25 points per call: evaluate a larger grid in chunks (``isosurface_chunk``)."""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _host
from ._host import _F, _I, _L, _P, _Z, guard as _guard, need_device as _need_device, ok as _ok, raw_stream as _raw_stream

_HEAD = [_P, _L, _I, _P, _P, _P, _I, _I, _I, _I]      # stream, N, n_input_dims, x, params, levels, n_levels, n_features, log2_hashmap_size, active_levels
SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_hashgrid_workspace_bytes": (_Z, [_L, _I, _I]),
    "tgs_hashgrid_encode": (_I, _HEAD + [_P]),
    "tgs_hashgrid_encode_backward": (_I, _HEAD + [_P, _P, _P, _P, _Z]),
    "tgs_hashgrid_field": (_I, _HEAD + [_P, _P, _P, _I, _I, _F, _P]),
    "tgs_hashgrid_field_backward": (_I, _HEAD + [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _Z]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_POINTS = 1 << 25
MAX_LEVELS = 16
FUSED_WIDTHS = (16, 32, 64)
MAX_OUT = 4

Level = collections.namedtuple("Level", "scale resolution size offset dense")


class _LevelRec(C.Structure):      # tgs_hashgrid_level_t
    _fields_ = [("scale", C.c_float), ("resolution", C.c_uint32), ("size", C.c_uint32), ("offset", C.c_uint32), ("dense", C.c_uint32)]


_IGNORED = ("start_level", "start_step", "update_steps", "include_xyz", "n_input_dims")
_DEFAULTS = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0, interpolation="Linear")


def _config(config) -> dict:
    """the keys this module needs of an encoding config, checked -> a plain dict"""
    if not hasattr(config, "get") or not hasattr(config, "keys"):
        raise RuntimeError(f"config must be a mapping, got {type(config).__name__}")
    otype = config.get("otype", "HashGrid")
    grid_type = config.get("type", "Hash")
    if otype not in ("HashGrid", "Grid", "ProgressiveBandHashGrid"):
        raise RuntimeError(f"otype {otype!r} is not served: the hash grid alone is (otype 'HashGrid', or 'Grid' with type 'Hash')")
    if otype == "Grid" and grid_type != "Hash":
        raise RuntimeError(f"a {grid_type!r} grid is not served: dense and tiled grids have no kernel here, type 'Hash' alone has")
    known = set(_DEFAULTS) | set(_IGNORED) | {"otype", "type"}
    unknown = sorted(set(config.keys()) - known)
    if unknown:
        raise RuntimeError(f"unknown keys in the encoding config: {unknown}")
    c = {k: config.get(k, v) for k, v in _DEFAULTS.items()}
    if c["n_features_per_level"] != 2:
        raise RuntimeError(f"n_features_per_level {c['n_features_per_level']} is not served: 2 features per level are")
    if c["interpolation"] != "Linear":
        raise RuntimeError(f"interpolation {c['interpolation']!r} is not served: 'Linear' is")
    if isinstance(c["n_levels"], bool) or not isinstance(c["n_levels"], int) or not 1 <= c["n_levels"] <= MAX_LEVELS:
        raise RuntimeError(f"n_levels must be an int in [1, {MAX_LEVELS}], got {c['n_levels']!r}")
    if isinstance(c["log2_hashmap_size"], bool) or not isinstance(c["log2_hashmap_size"], int) or not 3 <= c["log2_hashmap_size"] <= 24:
        raise RuntimeError(f"log2_hashmap_size must be an int in [3, 24], got {c['log2_hashmap_size']!r}")
    if not float(c["base_resolution"]) >= 1 or not float(c["per_level_scale"]) >= 1:
        raise RuntimeError(f"base_resolution and per_level_scale must be >= 1, got {c['base_resolution']!r} and {c['per_level_scale']!r}")
    return c


def level_table(config) -> list:
    """the encoding config -> the list of ``Level(scale, resolution, size, offset, dense)`` records, computed here once and never on the device.  For level
    l, in float32 arithmetic: ``scale = exp2(l * log2(per_level_scale)) * base_resolution - 1``, ``resolution = ceil(scale) + 1``;
    ``size = min(round_up(resolution^3, 8), 2^log2_hashmap_size)``; ``offset`` the running sum; ``dense = resolution^3 <= size``.  Pure numpy."""
    c = _config(config)
    f32 = np.float32
    out, offset = [], 0
    for l in range(c["n_levels"]):
        scale = f32(np.exp2(f32(l) * np.log2(f32(c["per_level_scale"]))) * f32(c["base_resolution"]) - f32(1.0))
        res = int(np.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << c["log2_hashmap_size"])
        out.append(Level(float(scale), res, size, offset, res ** 3 <= size))
        offset += size
    return out


def progressive_levels(config, global_step: int) -> int:
    """``ProgressiveBandHashGrid.update_step``'s schedule -> the ``active_levels`` of that step:
    ``min(start_level + max(global_step - start_step, 0) // update_steps, n_levels)``"""
    c = _config(config)
    return min(int(config["start_level"]) + max(int(global_step) - int(config["start_step"]), 0) // int(config["update_steps"]), c["n_levels"])


def _check_levels(levels, log2_hashmap_size: Optional[int] = None) -> int:
    """-> the number of entries"""
    if not isinstance(levels, (list, tuple)) or not 1 <= len(levels) <= MAX_LEVELS or not all(isinstance(v, Level) for v in levels):
        raise RuntimeError(f"levels must be a list of 1 to {MAX_LEVELS} Level records (level_table(config))")
    offset = 0
    for l, v in enumerate(levels):
        if v.offset != offset or v.size < 8 or v.size % 8 or v.size > 1 << 24 or v.resolution < 1 or not 0 <= v.scale < 2 ** 20 or (v.dense and v.resolution ** 3 > v.size) or \
                (log2_hashmap_size is not None and v.size > 1 << log2_hashmap_size):
            raise RuntimeError(f"level {l} of the table is inconsistent: {v}")
        offset += v.size
    return offset


def _log2_of(levels) -> int:
    return max(3, max(int(v.size - 1).bit_length() for v in levels))


def _records(levels):
    arr = (_LevelRec * len(levels))()
    for r, v in zip(arr, levels):
        r.scale, r.resolution, r.size, r.offset, r.dense = v.scale, v.resolution, v.size, v.offset, int(bool(v.dense))
    return arr


def _check_points(x) -> int:
    if not isinstance(x, torch.Tensor):
        raise RuntimeError("x must be a tensor")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"expected float32 x of shape [N,3], got {x.dtype} {tuple(x.shape)}")
    if x.shape[0] > MAX_POINTS:
        raise RuntimeError(f"x has {x.shape[0]} rows; at most 2^25 = {MAX_POINTS} points per call: evaluate the grid in chunks (isosurface_chunk)")
    return int(x.shape[0])


def _check_params(params, n_entries: int) -> None:
    if not isinstance(params, torch.Tensor):
        raise RuntimeError("params must be a tensor")
    if params.dtype != torch.float32 or params.dim() != 1 or params.shape[0] != 2 * n_entries:
        raise RuntimeError(f"expected float32 params of shape [{2 * n_entries}] (2 features for each of the table's {n_entries} entries), got {params.dtype} {tuple(params.shape)}")


def _check_active(active_levels, n_levels: int) -> int:
    if active_levels is None:
        return n_levels
    if isinstance(active_levels, bool) or not isinstance(active_levels, int) or not 0 <= active_levels <= n_levels:
        raise RuntimeError(f"active_levels must be None or an int in [0, {n_levels}], got {active_levels!r}")
    return active_levels


def _workspace(n_params: int, hidden: int, n_out: int, dev: torch.device):
    return _host.workspace(_lib.tgs_hashgrid_workspace_bytes(n_params, hidden, n_out), dev)


def _head(dev, N, x, params, levels, active):
    """the arguments every native call starts with; the record array is returned too, to keep it alive across the call"""
    recs = _records(levels)
    return recs, (_raw_stream(dev.index), N, 3, x.data_ptr(), params.data_ptr(), recs, len(levels), 2, _log2_of(levels), active)


# ---- the encoding ----------------------------------------------------------------------------------------------------------------------
def _encode_forward(x, params, levels, active, N, dev):
    enc = torch.empty((N, 2 * len(levels)), dtype=torch.float32, device=dev)
    if not N:
        return enc
    x, params = x.contiguous(), params.contiguous()
    with _guard(dev):
        recs, head = _head(dev, N, x, params, levels, active)
        _ok(_lib.tgs_hashgrid_encode(*head, enc.data_ptr()))
    return enc


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, levels, active, N, dev):
        ctx.args = (levels, active, N, dev)
        ctx.save_for_backward(x, params)
        return _encode_forward(x.detach(), params.detach(), levels, active, N, dev)

    @staticmethod
    @once_differentiable                                                       # a double backward (normal_type="analytic") raises
    def backward(ctx, g):
        x, params = ctx.saved_tensors
        levels, active, N, dev = ctx.args
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_x = d_p = None
        if not N:
            return (torch.zeros_like(x) if want_x else None, torch.zeros_like(params) if want_p else None) + (None,) * 4
        if want_x:
            d_x = torch.empty((N, 3), dtype=torch.float32, device=dev)
        if want_p:
            d_p = torch.empty_like(params, memory_format=torch.contiguous_format)
        if want_x or want_p:
            x, params, g = x.detach().contiguous(), params.detach().contiguous(), g.contiguous()
            with _guard(dev):
                ws, nbytes = _workspace(params.shape[0], 0, 0, dev)
                recs, head = _head(dev, N, x, params, levels, active)
                _ok(_lib.tgs_hashgrid_encode_backward(*head, g.data_ptr(), d_p.data_ptr() if want_p else None, d_x.data_ptr() if want_x else None, ws.data_ptr(), nbytes))
        return (d_x, d_p) + (None,) * 4


def hashgrid_encode(x: torch.Tensor, params: torch.Tensor, levels: Sequence[Level], active_levels: Optional[int] = None) -> torch.Tensor:
    """``x`` [N,3] float32 (the unit cube is the grid's domain), ``params`` [2 * entries] float32, the level table -> the encoding [N, 2 * n_levels]
    float32, differentiable with respect to ``params`` and, where ``x.requires_grad``, ``x`` (first order: the derivative of the trilinear weights).
    Columns of the levels at or above ``active_levels`` are exact zeros.  ``N = 0``: empty, no native call.  A double backward raises."""
    N = _check_points(x)
    n_entries = _check_levels(levels)
    _check_params(params, n_entries)
    active = _check_active(active_levels, len(levels))
    dev = _need_device("hashgrid", x=x, params=params)
    levels = tuple(levels)
    if torch.is_grad_enabled() and (x.requires_grad or params.requires_grad):
        return _Encode.apply(x, params, levels, active, N, dev)
    return _encode_forward(x.detach(), params.detach(), levels, active, N, dev)


class HashGrid(nn.Module):
    """``tcnn.Encoding(n_input_dims, config)`` for the hash grid: ``params`` (an ``nn.Parameter`` drawn from U(-1e-4, 1e-4), tiny-cuda-nn's layout),
    ``n_input_dims``, ``n_output_dims``, ``levels`` (the table; ``levels=`` overrides the one computed from the config) and
    ``forward(x, active_levels=None)``.  The schedule keys of ``ProgressiveBandHashGrid`` (``start_level``, ``start_step``, ``update_steps``) are ignored:
    its mask is ``active_levels``."""

    def __init__(self, n_input_dims: int, config, dtype=torch.float32, levels: Optional[Sequence[Level]] = None):
        super().__init__()
        if n_input_dims != 3:
            raise RuntimeError(f"n_input_dims {n_input_dims!r} is not served: 3 input dimensions are")
        if dtype != torch.float32:
            raise RuntimeError(f"dtype {dtype} is not served: float32 is (no half precision)")
        c = _config(config)
        self.levels = tuple(level_table(config) if levels is None else levels)
        n_entries = _check_levels(list(self.levels), c["log2_hashmap_size"])
        if len(self.levels) != c["n_levels"]:
            raise RuntimeError(f"levels has {len(self.levels)} records, the config {c['n_levels']} levels")
        self.n_input_dims, self.n_levels, self.n_output_dims = 3, len(self.levels), 2 * len(self.levels)
        self.params = nn.Parameter(torch.empty(2 * n_entries, dtype=torch.float32).uniform_(-1e-4, 1e-4))

    def forward(self, x: torch.Tensor, active_levels: Optional[int] = None) -> torch.Tensor:
        return hashgrid_encode(x, self.params, self.levels, active_levels)

    def extra_repr(self) -> str:
        return f"n_levels={self.n_levels}, n_params={self.params.numel()}"


# ---- the fused field -------------------------------------------------------------------------------------------------------------------
def _check_bbox(bbox):
    """-> None or (min[3], max[3]) as floats"""
    if bbox is None:
        return None
    b = np.asarray(bbox.detach().cpu() if isinstance(bbox, torch.Tensor) else bbox, dtype=np.float32)
    if b.shape != (2, 3) or not np.isfinite(b).all() or not (b[1] > b[0]).all():
        raise RuntimeError(f"bbox must be [2,3]: a finite min row below a max row, got {b.tolist()}")
    return tuple(map(float, b[0])), tuple(map(float, b[1]))


def _check_weights(W1, W2, n_cols: int):
    for name, w in (("W1", W1), ("W2", W2)):
        if not isinstance(w, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
        if w.dtype != torch.float32 or w.dim() != 2:
            raise RuntimeError(f"expected float32 {name} of two dimensions, got {w.dtype} {tuple(w.shape)}")
    H, D = int(W1.shape[0]), int(W2.shape[0])
    if W1.shape[1] != n_cols or W2.shape[1] != H:
        raise RuntimeError(f"expected W1 [H,{n_cols}] and W2 [D,H] as nn.Linear stores them, got {tuple(W1.shape)} and {tuple(W2.shape)}")
    if H not in FUSED_WIDTHS or not 1 <= D <= MAX_OUT:
        raise RuntimeError(f"the fused field serves a hidden width of 16, 32 or 64 and 1 to 4 outputs, got {H} and {D}: use SdfField, which falls back to hashgrid_encode and the torch layers")
    return H, D


def _field_tail(bbox, W1, W2, H, D):
    box = (C.c_float * 6)(*bbox[0], *bbox[1]) if bbox is not None else None
    return box, (box, W1.data_ptr(), W2.data_ptr(), H, D)


def _field_forward(x, params, W1, W2, levels, active, bbox, bias, N, H, D, dev):
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    if not N:
        return out
    x, params, W1, W2 = x.contiguous(), params.contiguous(), W1.contiguous(), W2.contiguous()
    with _guard(dev):
        recs, head = _head(dev, N, x, params, levels, active)
        box, tail = _field_tail(bbox, W1, W2, H, D)
        _ok(_lib.tgs_hashgrid_field(*head, *tail, bias, out.data_ptr()))
    return out


class _Field(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, W1, W2, levels, active, bbox, bias, N, H, D, dev):
        ctx.args = (levels, active, bbox, N, H, D, dev)
        ctx.save_for_backward(x, params, W1, W2)
        return _field_forward(x.detach(), params.detach(), W1.detach(), W2.detach(), levels, active, bbox, bias, N, H, D, dev)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, params, W1, W2 = ctx.saved_tensors
        levels, active, bbox, N, H, D, dev = ctx.args
        if ctx.needs_input_grad[0]:
            raise RuntimeError("the fused field has no gradient with respect to x: use hashgrid_encode and the torch layers where one is needed")
        want = ctx.needs_input_grad[1:4]
        if not N:
            return (None,) + tuple(torch.zeros_like(t) if w else None for t, w in zip((params, W1, W2), want)) + (None,) * 8
        outs = [torch.empty(t.shape, dtype=torch.float32, device=dev) if w else None for t, w in zip((params, W1, W2), want)]
        if any(want):
            x, params, W1, W2, g = x.detach().contiguous(), params.detach().contiguous(), W1.detach().contiguous(), W2.detach().contiguous(), g.contiguous()
            with _guard(dev):
                ws, nbytes = _workspace(params.shape[0], H, D, dev)
                recs, head = _head(dev, N, x, params, levels, active)
                box, tail = _field_tail(bbox, W1, W2, H, D)
                _ok(_lib.tgs_hashgrid_field_backward(*head, *tail, g.data_ptr(), *(o.data_ptr() if o is not None else None for o in outs), ws.data_ptr(), nbytes))
        return (None, *outs) + (None,) * 8


def sdf_field(x: torch.Tensor, params: torch.Tensor, levels: Sequence[Level], W1: torch.Tensor, W2: torch.Tensor, bbox=None, bias: float = 0.0,
              active_levels: Optional[int] = None) -> torch.Tensor:
    """The fused field: ``x`` [N,3] float32 -> ``W2 relu(W1 enc((x - bbox[0]) / (bbox[1] - bbox[0]))) + bias`` [N,D] float32, differentiable with respect
    to ``params``, ``W1`` [H, 2 * n_levels] and ``W2`` [D,H] (H in 16, 32, 64; D in 1..4), not to ``x``.  ``bbox=None``: ``x`` is taken as it is."""
    N = _check_points(x)
    n_entries = _check_levels(levels)
    _check_params(params, n_entries)
    active = _check_active(active_levels, len(levels))
    H, D = _check_weights(W1, W2, 2 * len(levels))
    bbox = _check_bbox(bbox)
    bias = float(bias)
    dev = _need_device("hashgrid", x=x, params=params, W1=W1, W2=W2)
    levels = tuple(levels)
    if torch.is_grad_enabled() and (x.requires_grad or params.requires_grad or W1.requires_grad or W2.requires_grad):
        return _Field.apply(x, params, W1, W2, levels, active, bbox, bias, N, H, D, dev)
    return _field_forward(x.detach(), params.detach(), W1.detach(), W2.detach(), levels, active, bbox, bias, N, H, D, dev)


def _fusable(mlp: nn.Module):
    """-> (W1, W2) of a bias-free Linear, ReLU, Linear network of a width the kernel covers and no output activation, else None"""
    act = getattr(mlp, "output_activation", None)
    probe = torch.tensor([-2.0, 0.0, 0.5])
    if act is not None and not (callable(act) and torch.equal(act(probe.clone()), probe)):      # (the reference's get_activation(None) is `lambda x: x`)
        return None
    body = getattr(mlp, "layers", mlp)
    mods = list(body) if isinstance(body, (nn.Sequential, list, tuple)) else None
    if mods is None or len(mods) != 3:
        return None
    a, r, b = mods
    if not (isinstance(a, nn.Linear) and isinstance(r, nn.ReLU) and isinstance(b, nn.Linear)) or a.bias is not None or b.bias is not None:
        return None
    if a.out_features not in FUSED_WIDTHS or not 1 <= b.out_features <= MAX_OUT or a.weight.dtype != torch.float32:
        return None
    return a.weight, b.weight


class SdfField(nn.Module):
    """``forward_sdf``: ``SdfField(encoding, W1, W2, bbox=None, bias=0.0)`` with the two weight matrices of the reference's ``VanillaMLP`` as they are
    stored (``layers[0].weight``, ``layers[2].weight``), or ``SdfField(encoding, mlp, bbox=..., bias=...)`` with the network itself.  ``fused`` tells
    which path ``forward(x, active_levels=None)`` takes: the fused kernel for a bias-free Linear, ReLU, Linear network of width 16, 32 or 64 and 1 to 4
    outputs; anything else (more hidden layers, other widths, layer biases, an output activation) goes through ``hashgrid_encode`` and the torch
    layers, which keeps the encoding on HIP.  ``bbox`` [2,3] is ``contract_to_unisphere``'s box (``unbounded=False``), ``bias`` is ``sdf_bias``."""

    def __init__(self, encoding: HashGrid, W1, W2=None, bbox=None, bias: float = 0.0):
        super().__init__()
        if not isinstance(encoding, HashGrid):
            raise RuntimeError(f"encoding must be a HashGrid, got {type(encoding).__name__}")
        self.encoding, self.bbox, self.bias, self.mlp = encoding, _check_bbox(bbox), float(bias), None
        if isinstance(W1, nn.Module):
            if W2 is not None:
                raise RuntimeError("give the network, or its two weight matrices, not both")
            pair = _fusable(W1)
            self.fused = pair is not None
            if self.fused:
                self.W1, self.W2 = pair
            else:
                self.mlp = W1
        else:
            _check_weights(W1, W2, encoding.n_output_dims)
            self.fused = True
            self.W1 = W1 if isinstance(W1, nn.Parameter) else nn.Parameter(W1)
            self.W2 = W2 if isinstance(W2, nn.Parameter) else nn.Parameter(W2)

    def forward(self, x: torch.Tensor, active_levels: Optional[int] = None) -> torch.Tensor:
        if self.fused:
            return sdf_field(x, self.encoding.params, self.encoding.levels, self.W1, self.W2, self.bbox, self.bias, active_levels)
        _check_points(x)
        if self.bbox is not None:
            mn, mx = (torch.tensor(b, dtype=torch.float32, device=x.device) for b in self.bbox)
            x = (x - mn) / (mx - mn)
        return self.mlp(self.encoding(x, active_levels)) + self.bias
