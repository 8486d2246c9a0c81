"""Marching tetrahedra for the geometry stage: the isosurface of an SDF on a tetrahedral grid, with gradients.

``marching_tets(pos, sdf, tet)`` returns what ``MarchingTetrahedraHelper._forward`` (``tetgs_spatial/models/isosurface.py`` :112-184) returns, so
that method's body becomes one ``return``; ``marching_tetrahedra(vertices, tets, sdf, return_tet_idx)`` has the call shape of the two third-party
calls of ``models/geometry/base.py`` (:350, :465), which need one changed import.  The kernels are ``csrc/tgs_marching_tets.hip``; the rules are
written down in include/tgs_raster.h, "marching tetrahedra", and restated in tests/mt_ref.py.  HIP device only: there is no CPU path.

What differs from the reference's thirty framework ops: the call reads back a handful of integers twice (the numbers of one- and two-triangle
tetrahedra with the index flag, then the number of mesh vertices) and nothing else crosses to the host; an index outside ``[0, N)`` raises
instead of faulting; two runs give the same bits, forward and backward.  ``marching_tetrahedra`` claims the third-party function's call shape
and ``_forward``'s rules (it has the same algorithm and provenance), not equality with that library's arithmetic, which is not available to
compare with.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _host
from ._host import _I, _L, _P, _Z, guard as _guard, index_error as _index_error, index_rows as _index_rows, ok as _ok, raw_stream as _raw_stream, workspace as _workspace

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_marching_tets_workspace_bytes": (_Z, [_I, _I]),
    "tgs_marching_tets_table_bytes": (_Z, [_L]),
    "tgs_marching_tets_classify": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _Z]),
    "tgs_marching_tets_edges": (_I, [_P, _I, _I, _P, _I, _L, _L, _P, _P, _Z, _P, _Z]),
    "tgs_marching_tets_emit": (_I, [_P, _I, _I, _P, _P, _P, _I, _L, _L, _L, _P, _P, _P, _P, _P, _Z, _P, _Z]),
    "tgs_marching_tets_backward_workspace_bytes": (_Z, [_I, _L]),
    "tgs_marching_tets_backward": (_I, [_P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _Z]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_ROWS = (1 << 31) - 1
MASK_TYPES = {torch.int32: 0, torch.int64: 1, torch.float32: 2, torch.uint8: 3, torch.bool: 3}     # what a keep / edit mask of ``tet_grid`` may be stored as
KEYS = ("verts", "faces", "face_to_tet_idx", "valid_tets", "interp_v")


def check(module_name: str, named, N: Optional[int] = None, each: bool = False) -> torch.device:
    """The argument check of the calls on a tetrahedral grid, here and in ``tet_grid``.  ``named``: (name, tensor, kind) with kind in pos / sdf / tet /
    mask; ``N``: the rows sdf and mask must have.  Types, then shapes and dtypes with the row limit, then the device -> the one device of all of them.
    ``each``: the row limit is said once for the first and the last tensor, behind every shape."""
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
    for name, t, kind in named:
        got = f"got {t.dtype} {tuple(t.shape)}"
        if kind == "pos" and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3):
            raise RuntimeError(f"expected float32 {name} of shape [N,3], {got}")
        if kind == "sdf" and (t.dtype != torch.float32 or tuple(t.shape) not in ((N,), (N, 1))):
            raise RuntimeError(f"expected float32 {name} of shape [{N}] or [{N},1], {got}")
        if kind == "tet" and (t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != 4):
            raise RuntimeError(f"expected int32 or int64 {name} of shape [F,4], {got}")
        if kind == "mask" and (t.dtype not in MASK_TYPES or tuple(t.shape) not in ((N,), (N, 1))):
            raise RuntimeError(f"expected an int32, int64, float32 or one-byte {name} of shape [{N}] or [{N},1], {got}")
        if not each and t.shape[0] > MAX_ROWS:
            raise RuntimeError(f"{name} has {t.shape[0]} rows; at most 2^31 - 1")
    (a, ta, _), (b, tb, _) = named[0], named[-1]
    if each and (ta.shape[0] > MAX_ROWS or tb.shape[0] > MAX_ROWS):
        raise RuntimeError(f"{a} has {ta.shape[0]} rows and {b} {tb.shape[0]}; at most 2^31 - 1 each")
    return _host.need_device(module_name, **{name: t for name, t, _ in named})


def _check(pos: torch.Tensor, sdf: torch.Tensor, tet: torch.Tensor) -> torch.device:
    """types, shapes and dtypes, then the device: everything that can be said before a native call -> the device"""
    return check("marching_tets", (("pos", pos, "pos"), ("sdf", sdf, "sdf"), ("tet", tet, "tet")), int(pos.shape[0]) if isinstance(pos, torch.Tensor) and pos.dim() else None, each=True)


def _forward(pos: torch.Tensor, sdf: torch.Tensor, tet: torch.Tensor, dev: torch.device):
    """checked, detached inputs -> (verts, faces, face_to_tet_idx, valid_tets, interp_v); two read-backs"""
    N, F = int(pos.shape[0]), int(tet.shape[0])
    pos, sdf, tet = pos.contiguous(), sdf.reshape(-1).contiguous(), _index_rows(tet)
    is64 = int(tet.dtype == torch.int64)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    valid = new((F,), torch.bool)
    empty = lambda: (new((0, 3), torch.float32), new((0, 3), torch.int64), new((0,), torch.int64), valid, new((0, 2), torch.int64))
    if F == 0:
        return empty()
    with _guard(dev):
        st = _raw_stream(dev.index)
        counts = new((4,), torch.int64)
        ws, nbytes = _workspace(_lib.tgs_marching_tets_workspace_bytes(N, F), dev)
        _ok(_lib.tgs_marching_tets_classify(st, N, F, sdf.data_ptr(), tet.data_ptr(), is64, valid.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes))
        n_one, n_two, bad, _ = counts.tolist()                                  # the first read-back
        if bad:
            raise _index_error("tet", N, f"pos has {N} rows")
        if n_one + n_two == 0:
            return empty()
        table, tbytes = _workspace(_lib.tgs_marching_tets_table_bytes(3 * n_one + 4 * n_two), dev)
        _ok(_lib.tgs_marching_tets_edges(st, N, F, tet.data_ptr(), is64, n_one, n_two, counts.data_ptr(), ws.data_ptr(), nbytes, table.data_ptr(), tbytes))
        M = int(counts[3].item())                                               # the second read-back
        T = n_one + 2 * n_two
        verts, interp_v, faces, f2t = new((M, 3), torch.float32), new((M, 2), torch.int64), new((T, 3), torch.int64), new((T,), torch.int64)
        _ok(_lib.tgs_marching_tets_emit(st, N, F, pos.data_ptr(), sdf.data_ptr(), tet.data_ptr(), is64, n_one, n_two, M, verts.data_ptr(), interp_v.data_ptr(),
                                        faces.data_ptr(), f2t.data_ptr(), ws.data_ptr(), nbytes, table.data_ptr(), tbytes))
    return verts, faces, f2t, valid, interp_v


class _MarchingTets(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, sdf, tet):
        ctx.dev = _check(pos, sdf, tet)
        out = _forward(pos.detach(), sdf.detach(), tet, ctx.dev)
        ctx.save_for_backward(pos, sdf, out[4])
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g_verts, *_):
        pos, sdf, interp_v = ctx.saved_tensors
        need_pos, need_sdf = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_pos or need_sdf):
            return None, None, None
        dev, N, M = ctx.dev, int(pos.shape[0]), int(interp_v.shape[0])
        d_pos = torch.empty((N, 3), dtype=torch.float32, device=dev) if need_pos else None
        d_sdf = torch.empty((N,), dtype=torch.float32, device=dev) if need_sdf else None
        with _guard(dev):
            ws, nbytes = _workspace(_lib.tgs_marching_tets_backward_workspace_bytes(N, M), dev)
            p, s, g = pos.detach().contiguous(), sdf.detach().reshape(-1).contiguous(), g_verts.contiguous()
            _ok(_lib.tgs_marching_tets_backward(_raw_stream(dev.index), N, M, p.data_ptr(), s.data_ptr(), interp_v.data_ptr(), g.data_ptr(),
                                                d_pos.data_ptr() if need_pos else None, d_sdf.data_ptr() if need_sdf else None, ws.data_ptr(), nbytes))
        return d_pos, d_sdf.reshape(sdf.shape) if need_sdf else None, None


def marching_tets(pos: torch.Tensor, sdf: torch.Tensor, tet: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``pos`` [N,3] float32, ``sdf`` [N] or [N,1] float32, ``tet`` [F,4] int32 or int64, on one HIP device -> the dict of ``_forward``:
    ``verts`` [M,3] float32, ``faces`` [T,3] int64, ``face_to_tet_idx`` [T] int64, ``valid_tets`` [F] bool, ``interp_v`` [M,2] int64.
    ``verts`` is differentiable with respect to ``pos`` and ``sdf``; the integer outputs are marked non-differentiable.  Under ``no_grad``, or
    with no input requiring a gradient, it is the forward alone.  Empty results have the shapes [0,3], [0,3], [0], [0,2]."""
    if torch.is_grad_enabled() and isinstance(pos, torch.Tensor) and isinstance(sdf, torch.Tensor) and (pos.requires_grad or sdf.requires_grad):
        out = _MarchingTets.apply(pos, sdf, tet)
    else:
        dev = _check(pos, sdf, tet)
        out = _forward(pos.detach(), sdf.detach(), tet, dev)
    return dict(zip(KEYS, out))


def marching_tetrahedra(vertices: torch.Tensor, tets: torch.Tensor, sdf: torch.Tensor, return_tet_idx: bool = False):
    """``vertices`` [B,N,3], ``tets`` [F,4], ``sdf`` [B,N] or [B,N,1] -> (list of verts, list of faces[, list of tet_idx]), one entry per batch
    element, each from ``marching_tets`` (a loop over B; the geometry stage has B = 1)."""
    if not isinstance(vertices, torch.Tensor) or not isinstance(sdf, torch.Tensor) or vertices.dim() != 3 or sdf.dim() not in (2, 3) or sdf.shape[0] != vertices.shape[0]:
        got = lambda t: f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"expected vertices of shape [B,N,3] and sdf of shape [B,N] or [B,N,1], got {got(vertices)} and {got(sdf)}")
    verts: List[torch.Tensor] = []
    faces: List[torch.Tensor] = []
    tet_idx: List[torch.Tensor] = []
    for b in range(int(vertices.shape[0])):
        out = marching_tets(vertices[b], sdf[b], tets)
        verts.append(out["verts"]); faces.append(out["faces"]); tet_idx.append(out["face_to_tet_idx"])
    return (verts, faces, tet_idx) if return_tet_idx else (verts, faces)
