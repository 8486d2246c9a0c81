"""The multi-view step of the rasterizer on one GPU: ``SyncFreeBatch`` renders and back-propagates the views of a step without a host
synchronisation per frame (``run_views``: three trips into the native library per step; ``run``: one rasterizer call per view), with the
fused gradient accumulation of ``rasterize_accumulate`` / ``DeferredBackward`` underneath.

The data-parallel host side -- ``shard_views``, ``FlatGradients``, ``render_batch_sharded`` -- lives in ``sharding`` and is re-exported
here, where callers have always imported it from.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Callable, Iterable, List, Optional, Sequence

import os
import threading

import torch

from .diff_gaussian_rasterization import _C
from .sharding import FlatGradients, _PackedReduce, _coalesced_all_reduce_supported, render_batch_sharded, shard_views  # noqa: F401


def _grad_buffers(leaves: dict) -> dict:
    """The ``.grad`` buffers the fused backward adds into: of every tensor of ``leaves`` that has elements and requires a gradient."""
    into = {}
    for name, t in leaves.items():
        if t.numel() and t.requires_grad:
            if not t.is_leaf or t.grad is None:
                raise RuntimeError(f"rasterize_accumulate: {name} must be a leaf parameter with an allocated .grad (see FlatGradients)")
            into[name] = t.grad
    return into


class DeferredBackward:
    """Collects the views of a batch whose backward has only run its per-pixel half (tgs_backward_render); ``finish`` runs
    the per-Gaussian half for all of them in one pass (tgs_backward_batch) and adds the result into the parameters'
    ``.grad`` buffers.  Reading the SH rows and read-modify-writing ``dL_dsh`` once per batch instead of once per view
    removes about two thirds of that pass's memory traffic."""

    def __init__(self):
        self.views: List[dict] = []
        self.leaves = None
        self.meta = None            # (sh_degree, scale_modifier)

    def add(self, rs, leaves, radii, geom, binning, img, R, means2D):
        key = tuple((k, t.data_ptr(), tuple(t.shape)) for k, t in leaves.items())
        if self.leaves is None:
            self.leaves, self._key, self.meta = leaves, key, (rs.sh_degree, rs.scale_modifier)
        elif key != self._key or self.meta != (rs.sh_degree, rs.scale_modifier):
            raise RuntimeError("DeferredBackward: all views of a batch must render the same parameter tensors with the same SH degree / scale modifier")
        self.views.append(dict(viewmatrix=rs.viewmatrix, projmatrix=rs.projmatrix, campos=rs.campos, tanfovx=rs.tanfovx, tanfovy=rs.tanfovy,
                               image_height=rs.image_height, image_width=rs.image_width, radii=radii, geom=geom, binning=binning, img=img, R=R,
                               means2D=means2D))

    def finish(self) -> None:
        if not self.views:
            return
        L = self.leaves
        if L["colors_precomp"].numel():
            raise RuntimeError("DeferredBackward supports the SH path (per-view colours have per-view gradients)")
        into = _grad_buffers(L)
        st = torch.cuda.current_stream()
        for v in self.views:                                 # buffers that were allocated on another stream of the batch
            for k in ("radii", "geom", "binning", "img"):
                v[k].record_stream(st)
        outs = _C.rasterize_gaussians_backward_batch(self.views, L["means3D"].detach(), L["sh"].detach(), self.meta[0], L["scales"].detach(),
                                                     L["rotations"].detach(), self.meta[1], L["cov3D_precomp"].detach(), into, accumulate=True)
        for v, (g2d, _gcol) in zip(self.views, outs):
            m = v["means2D"]
            if m is not None and m.requires_grad:
                m.grad = g2d if m.grad is None else m.grad + g2d
        self.views = []


_collector = threading.local()      # .batch: the DeferredBackward of the SyncFreeBatch.run that renders views on this thread


class _RasterizeAccumulate(torch.autograd.Function):
    """Rasterizer call for multi-view batches: identical forward; the backward ADDS the parameter gradients
    straight into the ``.grad`` tensors of the leaf parameters (tgs_backward_accumulate) instead of returning them
    for autograd to add in a second pass.  Every differentiable input must be a leaf that already has a ``.grad``
    buffer (e.g. from FlatGradients); ``means2D`` keeps its ordinary per-view gradient."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, r_capacity):
        rs = raster_settings
        from . import diff_gaussian_rasterization as dgr
        key = (int(means3D.shape[0]), int(rs.image_height), int(rs.image_width), means3D.device)
        guess = dgr._speculation.guess(key) if (dgr._SPECULATE and r_capacity is None) else None      # like GaussianRasterizer: read-back off the critical path
        out = _C.rasterize_gaussians(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix, rs.projmatrix,
            rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug,
            r_capacity=r_capacity, r_guess=guess)
        num_rendered, color, radii, geom, binning, img = out[:6]
        if dgr._SPECULATE and r_capacity is None:
            dgr._speculation.update(key, out[6] if guess is not None else num_rendered, guess)     # (out[6]: the true count, out[7]: tiles with instances)
        ctx.rs, ctx.num_rendered = rs, num_rendered         # sync-free: the binning capacity (what the buffers are carved for)
        ctx.collector = getattr(_collector, "batch", None) if (r_capacity is not None and colors_precomp.numel() == 0) else None
        ctx.means2D = means2D
        ctx.leaves = dict(means3D=means3D, sh=sh, colors_precomp=colors_precomp, opacities=opacities, scales=scales, rotations=rotations,
                          cov3D_precomp=cov3Ds_precomp)
        ctx.save_for_backward(radii, geom, binning, img)
        meta = _C.frame_meta(img) if img.numel() else torch.zeros(_C.META_BYTES, dtype=torch.uint8, device=color.device)
        ctx.mark_non_differentiable(radii, meta)
        return color, radii, meta

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, _grad_meta=None):
        rs, L = ctx.rs, ctx.leaves
        radii, geom, binning, img = ctx.saved_tensors
        if ctx.collector is not None:
            # batch mode: only the per-pixel half now; DeferredBackward.finish does the per-Gaussian half for all views at once
            _C.rasterize_gaussians_backward_render(rs.bg, grad_out_color, ctx.num_rendered, binning, img, L["means3D"].size(0))
            ctx.collector.add(rs, L, radii, geom, binning, img, ctx.num_rendered, ctx.means2D)
            return None, None, None, None, None, None, None, None, None, None
        into = _grad_buffers(L)
        g2d = _C.rasterize_gaussians_backward_accumulate(
            rs.bg, L["means3D"].detach(), radii, L["colors_precomp"].detach(), L["scales"].detach(), L["rotations"].detach(), rs.scale_modifier,
            L["cov3D_precomp"].detach(), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, L["sh"].detach(), rs.sh_degree,
            rs.campos, geom, ctx.num_rendered, binning, img, rs.debug, into)
        return None, g2d, None, None, None, None, None, None, None, None


def rasterize_accumulate(raster_settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                         cov3D_precomp=None, r_capacity: Optional[int] = None, return_meta: bool = False):
    """``GaussianRasterizer(raster_settings)(...)`` with fused gradient accumulation (HIP device only).

    ``r_capacity``: render sync-free (tgs_forward_async) with room for that many tile instances -- use through
    ``SyncFreeBatch``, which checks every frame afterwards and re-renders rejected ones.  ``return_meta`` appends the
    frame's 64-byte Meta record (device tensor, see ``_C.decode_meta``)."""
    e = torch.Tensor([])
    color, radii, meta = _RasterizeAccumulate.apply(
        means3D, means2D, e if shs is None else shs, e if colors_precomp is None else colors_precomp, opacities,
        e if scales is None else scales, e if rotations is None else rotations, e if cov3D_precomp is None else cov3D_precomp,
        raster_settings, r_capacity)
    return (color, radii, meta) if (return_meta or r_capacity is not None) else (color, radii)


_SIDE_STREAMS: dict = {}      # device -> [torch.cuda.Stream]: the side streams of all SyncFreeBatch objects (see _lanes)
_SIDE_LOCK = threading.Lock()


def _lanes(main: torch.cuda.Stream, n: int) -> list:
    """The ``n`` streams a batch spreads its views over: ``main`` and the first n - 1 side streams of its device."""
    # Side streams are shared by every SyncFreeBatch of the process (round 6): HIP multiplexes streams onto a few hardware queues, and a process that
    # had created a dozen of them -- bench.py's secondary workloads each built a batch object of their own -- ran its later batches up to 10 % slower
    # than a fresh process did (streams aliasing onto one queue: less overlap between the views).  A trainer has one batch object; this keeps it so.
    with _SIDE_LOCK:
        side = _SIDE_STREAMS.setdefault(main.device, [])
        while len(side) < n - 1:
            side.append(torch.cuda.Stream(device=main.device))
        return [main] + side[:n - 1]


def _fork(lanes: list) -> None:
    """The side lanes wait for what the first lane (the calling stream) holds."""
    ev = torch.cuda.Event()
    ev.record(lanes[0])
    for st in lanes[1:]:
        st.wait_event(ev)


def _join(lanes: list) -> None:
    """The first lane waits for what the side lanes hold."""
    for st in lanes[1:]:
        ev = torch.cuda.Event()
        ev.record(st)
        lanes[0].wait_event(ev)


def _read_verdicts(ready: Sequence[torch.cuda.Event], host: torch.Tensor) -> list:
    """The one host wait of a batch -- for the events ``ready``, behind which its Meta records are in the pinned rows ``host`` [V, 64] --
    and the records decoded: per view (R, rejected, (tiles with instances, tiles with >= 1024, tiles with >= 128 of them))."""
    for ev in ready:
        ev.synchronize()
    rows = []
    for meta in host:
        R, flags, _longest, _n_overflow = _C.decode_meta_full(meta)
        # (a tile list longer than the LDS sort is no reason to reject a frame any more: k_tile_sort's overflow workers sort it on the device)
        if flags & _C.FRAME_PREFILTERED:
            raise RuntimeError("Point is filtered although prefiltered is set. This shouldn't happen!")
        rows.append((R, bool(flags & _C.FRAME_REJECTED), _C.decode_meta_tiles(meta)))
    return rows


# A checked SyncFreeBatch.run_views call.  M: SH coefficients per Gaussian (0: per-view colours); precomp: per-view colours instead of SH;
# dsh_plane > 0: shs.grad is level-major, its coefficient planes this many floats apart; params: the leaves whose .grad the batch writes
# (means3D, opacities, scales, rotations, + sh); colors: colors_precomp [V,P,3], detached; ranges: (first, count) of the per-Gaussian
# launches, multiples of 256 Gaussians, the same on every rank.  The extra outputs: names: the maps asked for, of "alpha", "depth", "features",
# in the order of the return value and of the upstream callables' tuples; Cf: the feature channels (0: none); features: [P,Cf], detached;
# fgrad: features.grad where dL/d features goes, None when the features need no gradient.
_Call = namedtuple("_Call", "settings V P H W D M precomp dsh_plane params colors ranges names Cf features fgrad")


def _check_call(settings, means3D, opacities, shs, scales, rotations, upstream_batch, upstream_view, colors_precomp, grad_chunks,
                return_alpha=False, return_depth=False, features=None) -> _Call:
    """Checks the arguments of ``SyncFreeBatch.run_views``, the consistency of the views' settings first, the features last."""
    rs0 = settings[0]
    V, P, H, W, D = len(settings), int(means3D.size(0)), int(rs0.image_height), int(rs0.image_width), int(rs0.sh_degree)
    for rs in settings:
        if (int(rs.image_height), int(rs.image_width), int(rs.sh_degree)) != (H, W, D) or rs.scale_modifier != rs0.scale_modifier or \
                bool(rs.prefiltered) != bool(rs0.prefiltered):
            raise RuntimeError("run_views: all views of a batch share image size, SH degree, scale modifier and the prefiltered flag")
    precomp = colors_precomp is not None
    if (upstream_batch is None) == (upstream_view is None):
        raise RuntimeError("run_views: provide exactly one of upstream_batch / upstream_view")
    if precomp == (shs is not None):
        raise RuntimeError("run_views: provide exactly one of shs / colors_precomp")
    params = dict(means3D=means3D, opacities=opacities, scales=scales, rotations=rotations)
    if precomp:
        colors_precomp = colors_precomp.detach()
        if not (colors_precomp.is_cuda and colors_precomp.dtype == torch.float32 and colors_precomp.is_contiguous()
                and tuple(colors_precomp.shape) == (V, P, 3)):
            raise RuntimeError("run_views: colors_precomp must be a contiguous float32 GPU tensor [V,P,3]")
    else:
        params["sh"] = shs
    M = 0 if precomp else int(shs.size(1))
    # dL_dsh level-major (FlatGradients(level_major=True)): .grad is the [P, M, 3] view of M planes, strides (3, plane, 1)
    dsh_plane = 0
    if not precomp and shs.grad is not None and not shs.grad.is_contiguous():
        st = shs.grad.stride()
        if not (M == 16 and st[0] == 3 and st[2] == 1 and st[1] >= 3 * P and st[1] % 4 == 0 and shs.grad.data_ptr() % 16 == 0):
            raise RuntimeError("run_views: shs.grad must be contiguous, or the level-major view FlatGradients(level_major=True) makes of a [P,16,3] parameter")
        dsh_plane = int(st[1])
    for name, t in params.items():
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.is_leaf and t.grad is not None and
                (t.grad.is_contiguous() or (name == "sh" and dsh_plane))):
            raise RuntimeError(f"run_views: {name} must be a contiguous float32 leaf parameter on the GPU with an allocated .grad (see FlatGradients)")
    n_chunks = max(1, min(int(grad_chunks), (P + 255) // 256))
    per = ((P + n_chunks - 1) // n_chunks + 255) // 256 * 256
    ranges = [(first, min(per, P - first)) for first in range(0, P, per)]
    Cf = _check_features(features, P, means3D.device) if features is not None else 0
    names = [n for n, on in (("alpha", return_alpha), ("depth", return_depth), ("features", Cf)) if on]
    return _Call(settings, V, P, H, W, D, M, precomp, dsh_plane, params, colors_precomp, ranges, names, Cf,
                 features.detach() if Cf else None, features.grad if (Cf and features.requires_grad) else None)


def _check_features(features, P: int, dev: torch.device) -> int:
    """``run_views(features=)``: [P, C] float32, contiguous, on the model's device, 1 <= C <= 16; with requires_grad a leaf with an allocated
    ``.grad`` of the same shape (the rule of the parameters) -> C"""
    if not (torch.is_tensor(features) and features.dim() == 2 and int(features.size(0)) == P and features.dtype == torch.float32 and
            features.device == dev and features.is_contiguous() and 1 <= int(features.size(1)) <= _C.FEATURE_MAX_CHANNELS):
        raise RuntimeError(f"run_views: features must be a contiguous float32 tensor [P,C] on the model's device, 1 <= C <= {_C.FEATURE_MAX_CHANNELS}")
    if features.requires_grad and not (features.is_leaf and features.grad is not None and features.grad.shape == features.shape and
                                       features.grad.dtype == torch.float32 and features.grad.device == dev and features.grad.is_contiguous()):
        raise RuntimeError("run_views: features that require a gradient must be a leaf with an allocated contiguous .grad [P,C] (see FlatGradients)")
    return int(features.size(1))


def _upstream_checked(dL: torch.Tensor, c: _Call, require_gpu: bool = True) -> torch.Tensor:
    if not torch.is_tensor(dL) or dL.dtype != torch.float32 or (require_gpu and not dL.is_cuda) or tuple(dL.shape[-3:]) != (3, c.H, c.W):
        raise RuntimeError("upstream must return a float32 GPU tensor [V,3,H,W] or [3,H,W]")
    return dL.contiguous()


def _upstream_extras_checked(ret, c, names: Sequence[str], per_view: bool, require_gpu: bool = True, channels: Optional[dict] = None) -> tuple:
    """What an upstream callable returned when ``run_views`` handed it the maps ``names`` (of "alpha", "depth", "features", in that order):
    a tuple (dL/d images, dL/d map for every name), any of the latter None -> (dL, [gradient or None per name]), contiguous.
    ``channels``: the channel count of a map by its name (absent: 1, which alpha and depth have; "features": the C of the call).
    ``c`` needs H, W and V only; ``require_gpu=False`` checks everything but the device (host tests)."""
    want = "(dL_dimages, " + ", ".join("dL_d" + n for n in names) + ")"
    if not isinstance(ret, (tuple, list)) or len(ret) != 1 + len(names):
        raise RuntimeError(f"upstream must return the tuple {want} when run_views returns {' and '.join(names)} (an entry may be None, the first may not)")
    dL = _upstream_checked(ret[0], c, require_gpu)
    out = []
    for name, g in zip(names, ret[1:]):
        ch = int((channels or {}).get(name, 1))
        shapes = [(ch, c.H, c.W)] + ([] if per_view else [(c.V, ch, c.H, c.W)])
        if g is not None:
            if not torch.is_tensor(g) or g.dtype != torch.float32 or (require_gpu and not g.is_cuda) or tuple(g.shape) not in shapes:
                raise RuntimeError(f"upstream: dL_d{name} must be None or a float32 GPU tensor " + " or ".join(str(list(sh)) for sh in shapes[::-1]))
            g = g.contiguous()
        out.append(g)
    return dL, out


def _median_upstreams_checked(dL, c, require_gpu: bool = True) -> list:
    """The argument of ``SyncFreeBatch.backward_median_views`` -> per view its upstream gradient [1,H,W] (contiguous) or None.  ``dL``: a
    float32 GPU tensor [V,1,H,W], or [1,H,W] for all views, or a sequence of V entries, each [1,H,W] or None (that view takes no part).
    ``c`` needs H, W and V only; ``require_gpu=False`` checks everything but the device (host tests)."""
    one = (1, c.H, c.W)

    def ok(g, shapes):
        return torch.is_tensor(g) and g.dtype == torch.float32 and (g.is_cuda or not require_gpu) and tuple(g.shape) in shapes

    if torch.is_tensor(dL):
        if not ok(dL, [one, (c.V,) + one]):
            raise RuntimeError(f"backward_median_views: dL must be a float32 GPU tensor {[c.V] + list(one)} or {list(one)}, or a sequence of {c.V} such maps or None")
        dL = dL.contiguous()
        return [_of_view(dL, v) for v in range(c.V)]
    if not isinstance(dL, (tuple, list)) or len(dL) != c.V:
        raise RuntimeError(f"backward_median_views: dL must be a float32 GPU tensor {[c.V] + list(one)} or {list(one)}, or a sequence of {c.V} such maps or None")
    for v, g in enumerate(dL):
        if g is not None and not ok(g, [one]):
            raise RuntimeError(f"backward_median_views: dL[{v}] must be None or a float32 GPU tensor {list(one)}")
    return [None if g is None else g.contiguous() for g in dL]


def surface_votes(median_index: torch.Tensor, P: int, masks: Optional[torch.Tensor] = None, out=None):
    """Which Gaussians are the visible surface, over all views and without a read-back: ``median_index`` is the int32 map [V,1,H,W] (or
    [1,H,W]) of ``SyncFreeBatch.median_views`` / ``rasterize_gaussians(return_median=True)`` for a model of ``P`` Gaussians ->
    ``(seen, hits)``, int32 [P]: seen[p] = the number of pixels, over all views, whose surface is Gaussian p; hits[p] = the number of
    those that lie inside ``masks`` (``torch.bool`` or ``uint8``, the shape of ``median_index``; non-zero: inside) -- None without masks.
    Pixels without a surface (-1) vote for nobody.  ``out=(seen, hits)``: int32 [P] tensors the counts are ADDED to (hits: None without
    masks), so many cameras can be voted chunk by chunk; otherwise new zeroed tensors.  One kernel on the current stream (k_surface_votes:
    one integer atomic per run of equal indices in a wave); the counts do not depend on the order, two runs give the same bits.
    ``hits / seen`` above a threshold lifts 2-D edit masks to Gaussians."""
    if not (torch.is_tensor(median_index) and median_index.dtype == torch.int32 and median_index.dim() in (3, 4) and int(median_index.shape[-3]) == 1):
        raise RuntimeError("surface_votes: median_index must be an int32 tensor [V,1,H,W] or [1,H,W]")
    if masks is not None and not (torch.is_tensor(masks) and masks.dtype in (torch.bool, torch.uint8) and masks.shape == median_index.shape and
                                  masks.device == median_index.device):
        raise RuntimeError("surface_votes: masks must be a torch.bool or uint8 tensor of the shape and on the device of median_index")
    return _C.surface_votes(median_index.contiguous(), P, None if masks is None else masks.contiguous(), out)


def _of_view(dL: torch.Tensor, v: int) -> torch.Tensor:
    """View v's part of an upstream gradient ([3,H,W] / [1,H,W] / [C,H,W]: the same for every view; None stays None)."""
    return dL if (dL is None or dL.dim() == 3) else dL[v]


class _Upstream:
    """The upstream callables of one checked ``run_views`` call (built once per call): the one place that decides whether the extra maps
    are passed, checks what comes back and holds the view callable to [3,H,W].  Every route of ``run_views`` asks through it, so a wrong
    return fails with the same message on each.  ``c`` needs H, W, V, names and Cf only; ``require_gpu=False``: host tests."""

    def __init__(self, c, upstream_batch, upstream_view, require_gpu: bool = True):
        self.c, self.upstream_batch, self.upstream_view, self.require_gpu = c, upstream_batch, upstream_view, require_gpu
        self.per_view, self.channels = upstream_view is not None, {"features": c.Cf}

    def view(self, v: Optional[int], images: torch.Tensor, maps: Sequence[torch.Tensor]) -> tuple:
        """Asks for view v, on the current stream -> (dL/d image [3,H,W], the gradients of its extra maps in the order of ``c.names``, each
        [C,H,W] or None).  (``v`` None, for ``batch``: the batch callable, its gradients as they came, [V,...] or for all views.)"""
        c = self.c
        if v is None:
            ret = self.upstream_batch(images, *maps)
        elif maps:
            ret = self.upstream_view(v, images[v], *[m[v] for m in maps])
        else:
            ret = self.upstream_view(v, images[v])
        if c.names:
            dL, gs = _upstream_extras_checked(ret, c, c.names, v is not None, self.require_gpu, self.channels)
        else:
            dL, gs = _upstream_checked(ret, c, self.require_gpu), ()
        if v is not None and dL.dim() != 3:
            raise RuntimeError("upstream_view must return [3,H,W]")
        return dL, gs

    def batch(self, images: torch.Tensor, maps: Sequence[torch.Tensor]) -> tuple:
        """Asks for the whole batch -> (dL/d images, [V,3,H,W] or [3,H,W] for all views; per view the gradients of its extra maps, each
        [C,H,W] or None)."""
        dL, gs = self.view(None, images, maps)
        return dL, [[_of_view(g, v) for g in gs] for v in range(self.c.V)] if gs else [()] * self.c.V

    def views(self, images: torch.Tensor, maps: Sequence[torch.Tensor]) -> Callable[[int], tuple]:
        """For the routes that take the views one by one -> ``of(v) = (dL/d image, extra gradients)`` of view v: the batch callable is asked
        here, once; the view callable when ``of(v)`` is called."""
        if self.per_view:
            return lambda v: self.view(v, images, maps)
        dL, extra = self.batch(images, maps)
        return lambda v: (_of_view(dL, v), extra[v])


class SyncFreeBatch:
    """Renders the views of one step without a host synchronisation per frame.

    The reference's forward reads num_rendered back for every frame (rasterizer_impl.cu:280-281) and so does
    ``GaussianRasterizer``; between that read-back and the next launches the GPU idles.  A batch knows better: the
    instance count of a view changes slowly from step to step, so the binning buffer is sized from the counts seen so
    far (times ``headroom``) and nothing is read back until the batch is done.  Then ONE copy fetches every frame's
    Meta record; a frame that did not fit rendered as background and accumulated nothing (it was rejected on the
    device), and is rendered again with the synchronous forward, which also raises the bound.  Results are those of
    the synchronous path: only the binning capacity differs.

    ``rasterize(v, r_capacity)`` renders view ``v`` with ``rasterize_accumulate(..., r_capacity=r_capacity,
    return_meta=True)`` and returns its ``(image, radii, meta)``; ``upstream(v, image)`` returns dL/d image (it runs
    again for a re-rendered view)."""

    def __init__(self, headroom: float = 1.25, granule: int = 1 << 16, streams: int = 4, deferred: bool = True, split: bool = False,
                 deterministic: Optional[bool] = None, forward_group: int = 0, pruning: Optional[bool] = None, light_tiles: Optional[bool] = None):
        self.headroom, self.granule = float(headroom), int(granule)
        # explicit per-call options of the whole-batch entry points (tgs_options_t: the bitwise-reproducible per-pixel backward, views per
        # launch of the per-Gaussian forward stage, instance pruning, light tiles); None: the library's defaults -- no process-wide setter
        self.options = (_C.options(deterministic=deterministic, forward_group=forward_group, pruning=pruning, light_tiles=light_tiles)
                        if (deterministic is not None or forward_group or pruning is not None or light_tiles is not None) else None)
        self._deterministic, self._pruning = deterministic, pruning      # the per-view fallback path (first batch, re-rendered views) gets the same
        self.bound: Optional[int] = None        # largest num_rendered seen (decays slowly)
        self.tile_bound: Optional[int] = None   # largest number of tiles with instances seen (decays slowly): sizes the sync-free grids
        self.class_bound = [0, 0]               # the same for the tiles with >= 1024 / >= 128 instances (classes of the tile sort)
        self.rejected = 0                       # frames re-rendered so far
        self.streams = max(1, int(streams))     # 2: consecutive views alternate between two HIP streams (see run)
        self.deferred = bool(deferred)          # one per-Gaussian backward pass for the whole batch (DeferredBackward)
        # run_views(upstream_view=...): half of the streams bin (per-Gaussian forward .. finalize), the other half composite
        # (k_render_fwd, the loss, k_render_bwd): kernels bound by the L2 atomics / by latency next to kernels bound by VALU issue
        self.split = bool(split)
        self._host: Optional[torch.Tensor] = None
        self._cooldown = 0                      # batches left to render synchronously (unused since overflow lists are sorted on the device; kept for callers that set it)
        self._pool = None
        self.viewspace_grads: Optional[torch.Tensor] = None
        self.color_grads: Optional[torch.Tensor] = None      # run_views with colors_precomp: dL/d colours per view [V,P,3]
        self._last: Optional[dict] = None       # the last run_views call, for median_views / backward_median_views (references, no buffers)
        self._mpool: Optional[dict] = None      # the median maps [V,1,H,W] of median_views (allocated with its first call)

    def tile_capacity(self) -> int:
        """bound on the tiles with instances handed to the sync-free forward (0: none yet); a frame with more is rejected and rendered again"""
        if self.tile_bound is None or os.environ.get("TGS_TILE_BOUND", "1") == "0":      # (TGS_TILE_BOUND=0: grids over all tiles, for A/B runs)
            return 0
        return (int(self.tile_bound * 1.1) + 64) // 64 * 64

    def capacity(self) -> Optional[int]:
        if self.bound is None or self._cooldown > 0:
            return None
        c = int(self.bound * self.headroom) + 1
        return min(0x7fffffff, (c + self.granule - 1) // self.granule * self.granule)

    def _learn(self, seen: int, tiles: Optional[Sequence[int]] = None) -> None:
        """What a batch saw: the largest instance count of its views, and (sync-free frames) of tiles with instances, with >= 1024, with >= 128."""
        decayed = lambda bound, new: new if bound is None else max(new, int(bound * 0.95))
        self.bound = decayed(self.bound, seen)
        if tiles is not None:
            self.tile_bound = decayed(self.tile_bound, tiles[0])
            self.class_bound = [decayed(self.class_bound[0], tiles[1]), decayed(self.class_bound[1], tiles[2])]
        if self._cooldown > 0:
            self._cooldown -= 1

    # ------------------------------------------------------------------------------------------------------------------
    # Whole-batch path: three trips into the native library per batch (tgs_forward_views, tgs_backward_render_views,
    # tgs_backward_batch) instead of several per view.  Measured: the per-view path costs ~0.4 ms of Python, autograd and
    # launch time per frame -- as much as the GPU needs for the frame once the views overlap on several streams.
    # ------------------------------------------------------------------------------------------------------------------
    def run_views(self, settings: Sequence, means3D: torch.Tensor, opacities: torch.Tensor, shs: torch.Tensor, scales: torch.Tensor,
                  rotations: torch.Tensor, upstream_batch: Optional[Callable[[torch.Tensor], torch.Tensor]], accumulate: bool = True,
                  colors_precomp: Optional[torch.Tensor] = None,
                  upstream_view: Optional[Callable[[int, torch.Tensor], torch.Tensor]] = None, grad_chunks: int = 1,
                  on_chunk: Optional[Callable[[int, int], None]] = None, return_alpha: bool = False, return_depth: bool = False,
                  features: Optional[torch.Tensor] = None):
        """Renders the views described by ``settings`` (GaussianRasterizationSettings, same image size, SH degree and scale
        modifier) of one Gaussian model (leaf parameters with allocated ``.grad``, SH colours, scales + rotations), calls
        ``upstream_batch(images[V,3,H,W]) -> dL/d images`` ([V,3,H,W], or [3,H,W] for all views) ONCE, and adds the
        gradients of all views into the parameters' ``.grad`` (``accumulate=False``: overwrites them instead -- the
        step then needs no zeroing pass and the batch kernel no read of the old values).  Returns the images -- a view
        of a buffer the next call reuses; ``self.viewspace_grads`` [V,P,3] holds dL/d means2D per view.

        ``upstream_view(v, image[3,H,W]) -> dL/d image`` instead of ``upstream_batch`` (pass ``None`` for that): for losses that are
        sums over the views (the reference's are: refine.py:245-247 takes the loss of one image).  It is called per view under the
        HIP stream that view runs on, so a view's backward follows its own forward and loss without any cross-stream wait -- the
        streams meet only before the per-Gaussian pass (two event round trips per step instead of four, each ~20-40 us of idle
        GPU on this platform, and no phase boundary where every stream drains).

        ``colors_precomp`` [V,P,3] (float32, with ``shs=None``): the reference's training mode -- colours evaluated by the caller
        per view (``compute_color_in_rasterizer=False``, tetgs_model.py:524-537; e.g. ``sh_color.points_rgb``); their
        gradients come back in ``self.color_grads`` [V,P,3] for the caller's ``colors.backward(batch.color_grads)``.

        ``grad_chunks`` / ``on_chunk(first, count)``: the step's one per-Gaussian pass runs as ``grad_chunks`` launches over consecutive
        ranges of Gaussians, and ``on_chunk`` is called right behind each launch (on the calling stream) -- the parameter gradients of
        Gaussians [first, first + count) are final once that launch is: a data-parallel step starts their all-reduce there
        (``FlatGradients.all_reduce_rows``) while the next range is still being computed.

        ``return_alpha`` / ``return_depth``: the accumulated alpha (1 - final_T) and the expected depth (sum_i T_i alpha_i z_i, not
        normalised) of every view as well, with gradients -- the outputs of ``rasterize_gaussians(return_alpha=, return_depth=)`` in the
        whole-batch path.  ``run_views`` then returns ``(images, alpha[V,1,H,W] if asked, depth[V,1,H,W] if asked)`` (views of pooled
        buffers, like the images), the upstream callables receive the maps as further positional arguments in that order --
        ``upstream_batch(images, alpha, depth)``, ``upstream_view(v, image, alpha_v[1,H,W], depth_v[1,H,W])`` -- and return the tuple
        ``(dL/d images, dL/d alpha, dL/d depth)`` in the same order: float32 GPU tensors [V,1,H,W] or [1,H,W] (all views) from the batch
        callable, [1,H,W] from the view callable.  Any of the extra gradients may be None: that map took no part in the loss and no kernel
        runs for it.  Both flags False (the default): nothing changes -- the same calls, buffers and return value as before.

        ``features`` [P,C] (float32, contiguous, on the model's device, 1 <= C <= 16; anything else raises RuntimeError): per-Gaussian
        feature channels -- normals, keep / edit masks, labels: properties of the model, so one tensor for all views -- composited like the
        colour, the output of ``rasterize_gaussians(features=)`` in the whole-batch path: feature_map[v, c] = sum_i T_i alpha_i features[i, c]
        over the pairs view v's colour frame blended (signed, not clamped, not normalised).  ``run_views`` then returns
        ``(images, alpha if asked, depth if asked, feature_map[V,C,H,W])``, the upstream callables receive the feature map as the LAST
        positional argument -- ``upstream_batch(images, ..., fmap)``, ``upstream_view(v, image, ..., fmap_v[C,H,W])`` -- and return its gradient
        as the last entry of the tuple: [V,C,H,W] or [C,H,W] (all views) from the batch callable, [C,H,W] from the view callable, or None:
        the map took no part in that view's loss, no feature kernel runs for the view and it adds nothing to dL/d features.  If
        ``features.requires_grad`` it must be a leaf with an allocated ``.grad`` [P,C], the rule of the parameters, and dL/d features of all
        views is stored there (``accumulate=False``) or added; if not, ``.grad`` is not touched and only the through-alpha share of the
        gradient flows, to opacities, means, scales and rotations.  Memory: once a view has a feature gradient the pool holds a scratch of
        V * capacity * C * 4 bytes (capacity: the batch's bound on the tile instances of a view) -- large at C = 16: 8 views of a million
        instances are 512 MB.  ``features=None`` (the default) is the step of before: the same calls, buffers and return value.

        ``run`` / ``rasterize_accumulate`` / ``DeferredBackward`` carry none of these outputs (alpha, depth, feature channels); per-view
        features [V,P,C], more than 16 channels and half precision are not part of this path either.  The median depth and the surface index
        of the views are no argument of this call: ``median_views()`` and ``backward_median_views(dL)`` behind it."""
        c = _check_call(settings, means3D, opacities, shs, scales, rotations, upstream_batch, upstream_view, colors_precomp, grad_chunks, return_alpha, return_depth, features)
        self._last = None                                   # (and with it the synchronous frames median_views kept)
        ask = _Upstream(c, upstream_batch, upstream_view)
        cap = self.capacity()
        if cap is None:                                     # no bound yet: synchronous frames
            images, maps, seen = self._step_synchronous(c, ask, accumulate)
            tiles, eager = None, False
            last = dict(c=c, pool=None, sync=list(range(c.V)), chunked=on_chunk is not None)
        else:
            pool, rows, eager = self._step_pooled(c, ask, cap, accumulate, on_chunk)
            images, maps = pool["images"], [pool[name] for name in c.names]
            seen = max(R for R, _rejected, _tiles in rows)
            redo = [v for v, (_R, rejected, _tiles) in enumerate(rows) if rejected]
            if redo:
                self.rejected += len(redo)
                seen = max(seen, self._render_again(c, ask, pool, redo))
            tiles = [max(counts) for counts in zip(*(tiles for _R, _rejected, tiles in rows))]
            last = dict(c=c, pool=pool, cap=cap, sync=redo, chunked=on_chunk is not None)
        if on_chunk is not None and not eager:
            for first, count in c.ranges:     # the same calls in the same order as on a rank that had nothing to render again (collectives must pair up)
                on_chunk(first, count)
        self._learn(seen, tiles)
        self._last = last
        return (images, *maps) if c.names else images

    # ---- the three routes of run_views ----
    def _step_synchronous(self, c: _Call, ask: _Upstream, accumulate: bool) -> tuple:
        """The step of a batch that has no bound yet: every view through the synchronous forward, every loss, then every view's backward
        -> (images [V,3,H,W], the extra maps, the largest instance count)."""
        views = range(c.V)
        if not accumulate:
            for t in c.params.values():
                t.grad.zero_()
            if c.fgrad is not None:
                c.fgrad.zero_()
        states = [self._render_view(c, v) for v in views]
        images = torch.stack([s[1] for s in states])
        maps = [torch.stack([self._map_of(c, name, states[v]) for v in views]) for name in c.names]
        grads = list(map(ask.views(images, maps), views))   # (every loss in front of the first backward)
        z = lambda: torch.empty((c.V, c.P, 3), dtype=torch.float32, device=images.device)
        self.viewspace_grads, self.color_grads = z(), (z() if c.precomp else None)
        self._backward_views(c, views, states, grads.__getitem__, self.viewspace_grads, self.color_grads)
        return images, maps, max(s[0] for s in states)

    def _render_again(self, c: _Call, ask: _Upstream, pool: dict, redo: Sequence[int]) -> int:
        """The views ``redo`` of a pooled step, rejected on the device (they rendered the background and accumulated nothing): through the
        synchronous forward into their slices of the pooled images and maps, then loss and backward view by view -- the batch callable is
        asked again first: its gradients depend on the corrected frames -> the largest instance count."""
        states = {v: self._render_view(c, v) for v in redo}
        images, maps = pool["images"], [pool[name] for name in c.names]
        for v in redo:
            images[v].copy_(states[v][1])
            for name, m in zip(c.names, maps):
                m[v].copy_(self._map_of(c, name, states[v]))
        self._backward_views(c, redo, states, ask.views(images, maps), pool["g2d"], pool["gcol"])
        return max(states[v][0] for v in redo)

    def _backward_views(self, c: _Call, views: Sequence[int], states, grads_of: Callable[[int], tuple], g2d: torch.Tensor, gcol: Optional[torch.Tensor]) -> None:
        """The backward of synchronously rendered views, one after the other on the current stream: ``grads_of(v)`` gives view v's upstream
        gradients (_Upstream.views), its dL/d means2D lands in ``g2d[v]``, its colour gradients (per-view colours) in ``gcol[v]``."""
        scratch = torch.empty_like(c.params["sh"]) if c.dsh_plane else None
        for v in views:
            g, gs = grads_of(v)
            g2d[v].copy_(self._backward_view(c, v, states[v], g, gcol, scratch, gs))

    def _step_pooled(self, c: _Call, ask: _Upstream, cap: int, accumulate: bool, on_chunk) -> tuple:
        """The sync-free step on the pooled buffers, sized for ``cap`` instances per view: forward and extra outputs of every view on the
        lanes, the upstream callables, the per-pixel backward on the lanes, then the per-Gaussian pass range by range on the calling stream
        with ``on_chunk`` behind each range -> (the pool, the views' verdicts (_read_verdicts), whether on_chunk has been called)."""
        p, s0 = c.params, c.settings[0]
        means3D, opacities, scales, rotations, shs = p["means3D"], p["opacities"], p["scales"], p["rotations"], p.get("sh")
        V, P, D, M, precomp, names, fgrad = c.V, c.P, c.D, c.M, c.precomp, c.names, c.fgrad
        dev = means3D.device
        pool = self._pooled(c, cap)
        self._fill_views(c, pool)
        arr, images = pool["arr"], pool["images"]
        xarr, farr, maps = pool.get("xarr"), pool.get("farr"), [pool[name] for name in names]
        main = torch.cuda.current_stream(dev)
        lanes = _lanes(main, min(self.streams, V))
        with torch.cuda.device(dev):
            split = self.split and ask.per_view and len(lanes) >= 4
            bin_lanes, ren_lanes = (lanes[:len(lanes) // 2], lanes[len(lanes) // 2:]) if split else (lanes, lanes)
            _fork(lanes)
            _C.set_render_streams([st.cuda_stream for st in ren_lanes] if split else [])
            try:
                _C.forward_views([st.cuda_stream for st in bin_lanes], cap, P, D, M, means3D.data_ptr(), None if precomp else shs.data_ptr(), opacities.data_ptr(),
                                 scales.data_ptr(), s0.scale_modifier, rotations.data_ptr(), arr, V, prefiltered=s0.prefiltered, opt=self.options)
            finally:
                _C.set_render_streams([])
            if xarr is not None:
                # the maps read what k_render_fwd wrote: on the lane each view composited on, behind it without an event
                _C.outputs_views([st.cuda_stream for st in ren_lanes], P, arr, xarr, V)
            if farr is not None:
                _C.features_views([st.cuda_stream for st in ren_lanes], P, arr, farr, V)
            if not ask.per_view:
                _join(lanes)
                ready = [torch.cuda.Event()]                # (the verdicts are in pinned memory once the scans have run: tgs_view_t.host_meta)
                ready[0].record(main)
                dL, extra = ask.batch(images, maps)
                grads = [(v, _of_view(dL, v), extra[v]) for v in range(V)]
                self._keep = extra                          # (alive until the next batch)
                _fork(lanes)
            else:
                # every lane: the verdicts of its views leave for the host, then loss and backward of each view follow on the same stream
                ready, grads, ask_view = [], [], ask.view
                for st in bin_lanes:
                    with torch.cuda.stream(st):
                        ev = torch.cuda.Event()             # behind the lane's forwards: their scans have written the verdicts to pinned memory
                        ev.record(st)
                        ready.append(ev)
                for l, st in enumerate(ren_lanes):
                    with torch.cuda.stream(st):
                        for v in range(l, V, len(ren_lanes)):
                            g, gs = ask_view(v, images, maps)
                            g.record_stream(st)
                            for x in gs:
                                if x is not None:
                                    x.record_stream(st)
                            grads.append((v, g, gs))
                self._keep = grads                          # (alive until the next batch)
            for v, g, _gs in grads:
                arr[v].dL_dpix = g.data_ptr()
            # a view has a depth gradient: the z-path pass follows every range of the per-Gaussian pass; a feature gradient: dL/d features too
            with_depth, with_feat = self._set_extra_grads(c, pool, grads) if names else (False, False)
            bwd_lanes = [st.cuda_stream for st in (ren_lanes if ask.per_view else lanes)]
            if farr is not None:                            # colour + alpha, then depth, then the features' share, per view on its lane
                _C.backward_render_views_features(bwd_lanes, P, arr, xarr, farr, V, opt=self.options)
            elif names:
                _C.backward_render_views_extras(bwd_lanes, P, arr, xarr, V, opt=self.options)
            else:
                _C.backward_render_views(bwd_lanes, P, arr, V, opt=self.options)
            _join(lanes)
            # With on_chunk the verdict is read BEFORE the per-Gaussian pass is enqueued (the GPU still has the per-pixel backwards in its
            # queues): a range may only be handed out as final when no view has to be rendered again.
            rows = _read_verdicts(ready, pool["host"]) if on_chunk is not None else None
            eager = rows is not None and not any(rejected for _R, rejected, _tiles in rows)
            # the one per-Gaussian pass of the step, range by range: a range's gradients are final behind its launch
            for g0, gcount in c.ranges:
                _C.backward_batch_raw(main.cuda_stream, P, D, M, arr, V, means3D.data_ptr(), None if precomp else shs.data_ptr(), scales.data_ptr(),
                                      s0.scale_modifier, rotations.data_ptr(), opacities.grad.data_ptr(), means3D.grad.data_ptr(),
                                      None if precomp else shs.grad.data_ptr(), scales.grad.data_ptr(), rotations.grad.data_ptr(), accumulate, g0, gcount,
                                      dsh_plane_stride=c.dsh_plane)
                if with_depth:                              # dz . (third row of each view's transform), behind the range's stored / accumulated dL_dmeans3D
                    _C.backward_batch_depth_raw(main.cuda_stream, P, arr, xarr, V, means3D.grad.data_ptr(), g0, gcount)
                if fgrad is not None and (with_feat or not accumulate):      # (store mode without any gradient: the range's rows are zeroed)
                    _C.backward_batch_features_raw(main.cuda_stream, P, arr, farr, V, fgrad.data_ptr(), accumulate, g0, gcount)
                if eager:
                    on_chunk(g0, gcount)
        self.viewspace_grads, self.color_grads = pool["g2d"], pool["gcol"]
        return pool, (rows if rows is not None else _read_verdicts(ready, pool["host"])), eager

    # ------------------------------------------------------------------------------------------------------------------
    # The median of the batch's views: calls of their own behind run_views.  The forward reads what the step's forward kernels left in the
    # pooled frames (the step's backward writes none of it), the gradient reaches positions alone and replays nothing.
    # ------------------------------------------------------------------------------------------------------------------
    def median_views(self):
        """``(median_depth[V,1,H,W] float32, median_index[V,1,H,W] int32)`` of the views of the LAST ``run_views`` call on this object, from
        the frames that call left in the pool -- the outputs of ``rasterize_gaussians(return_median=True)`` for every view, bit for bit: the
        view-space z and the Gaussian index of the first blended splat behind which the transmittance is below one half; 0 / -1 where no
        surface exists.  Views of pooled buffers the next call reuses.  View k runs on lane k mod ``streams``, forked from and joined to the
        current stream; no host synchronisation.  RuntimeError before any ``run_views`` call.  The maps describe the parameters ``run_views``
        rendered: if they changed in between (an optimizer step), the results are undefined.

        Frames the pool does not hold -- every view of a synchronous batch (the first one: no bound yet) and views that were rendered again
        after a rejection -- are rendered once more by the synchronous forward from the inputs of the last call (kept by reference), and
        their states are kept until the next ``run_views``.  The first call allocates the three maps (12 bytes per pixel and view)."""
        last = self._last
        if last is None:
            raise RuntimeError("median_views: no finished run_views call on this object (call run_views first)")
        c, pool, sync = last["c"], last["pool"], last["sync"]
        V, P, H, W = c.V, c.P, c.H, c.W
        dev = c.params["means3D"].device
        key = (V, H, W, dev)
        if self._mpool is None or self._mpool["key"] != key:
            z = lambda dt: torch.empty((V, 1, H, W), dtype=dt, device=dev)
            self._mpool = dict(key=key, depth=z(torch.float32), index=z(torch.int32), pos=z(torch.int32), marr=_C.ViewMedianArray(V))
        mp = self._mpool
        for v in range(V):
            m, own = mp["marr"][v], v not in sync
            m.out_depth = mp["depth"][v].data_ptr() if own else None
            m.out_index = mp["index"][v].data_ptr() if own else None
            m.out_pos = mp["pos"][v].data_ptr() if own else None
            m.dL_dmedian_depth = m.dz_scratch = None
        with torch.cuda.device(dev):
            if pool is not None and len(sync) < V:
                lanes = _lanes(torch.cuda.current_stream(dev), min(self.streams, V))
                _fork(lanes)
                _C.median_views([st.cuda_stream for st in lanes], P, pool["arr"], mp["marr"], V)
                _join(lanes)
            states = last.setdefault("states", {})
            for v in sync:
                if v not in states:
                    states[v] = self._render_view(c, v)
                R, _color, _radii, geom, binning, img = states[v][:6]
                for name, t in zip(("depth", "index", "pos"), _C.median_from_state(geom, binning, img, P, H, W, int(R))):
                    mp[name][v].copy_(t)
        last["median"] = True
        return mp["depth"], mp["index"]

    def backward_median_views(self, dL) -> None:
        """Adds the gradient of the median depths of all views into ``means3D.grad``, behind whatever ``run_views`` stored or accumulated
        there (the median depth moves positions alone: d median_depth / d z of the median splat = 1, through the third row of each view's
        transform; nothing reaches opacities, scales, rotations or colours).  ``dL``: dL/d median_depth, a float32 GPU tensor [V,1,H,W], or
        [1,H,W] for all views, or a sequence of V entries, each [1,H,W] or None -- that view takes no part and no kernel runs for it;
        anything else raises RuntimeError.  Call it after ``median_views()`` of the same step.  Per view the per-pixel half runs on the
        lanes, then ONE pass over the Gaussians per range of the call (``grad_chunks``) on the current stream; views ``median_views`` had to
        render synchronously go through the one-view call.  The first call grows the pool by a float scratch [V, capacity].

        RuntimeError if the last ``run_views`` had ``on_chunk``: the gradients of its ranges were handed out as final (their all-reduce may
        be in flight) and must not be added to."""
        last = self._last
        if last is None or not last.get("median"):
            raise RuntimeError("backward_median_views: call median_views() after run_views first (its position maps are what this pass reads)")
        if last["chunked"]:
            raise RuntimeError("backward_median_views: the last run_views call had on_chunk -- its ranges were handed out as final")
        c, pool, sync, mp = last["c"], last["pool"], last["sync"], self._mpool
        gs = _median_upstreams_checked(dL, c)
        V, P, H, W = c.V, c.P, c.H, c.W
        means3D = c.params["means3D"]
        dev = means3D.device
        last["keep"] = gs                                   # (alive until the next batch)
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            own = [v for v in range(V) if v not in sync and gs[v] is not None]
            if own:
                if "mdz" not in pool:
                    pool["mdz"] = torch.empty((V, last["cap"]), dtype=torch.float32, device=dev)      # one float per instance slot and view
                for v in range(V):
                    m = mp["marr"][v]
                    m.dL_dmedian_depth = gs[v].data_ptr() if v in own else None
                    m.dz_scratch = pool["mdz"][v].data_ptr() if v in own else None
                lanes = _lanes(main, min(self.streams, V))
                _fork(lanes)
                _C.backward_median_views([st.cuda_stream for st in lanes], P, pool["arr"], mp["marr"], V)
                _join(lanes)
                for g0, gcount in c.ranges:
                    _C.backward_batch_median_raw(main.cuda_stream, P, pool["arr"], mp["marr"], V, means3D.grad.data_ptr(), g0, gcount)
            for v in sync:
                if gs[v] is None:
                    continue
                R, _color, radii, geom, binning, img = last["states"][v][:6]
                if int(R) == 0:
                    continue
                dz = torch.empty((int(R),), dtype=torch.float32, device=dev)
                _C.backward_median_raw(main.cuda_stream, P, W, H, int(R), geom.data_ptr(), binning.data_ptr(), img.data_ptr(),
                                       c.settings[v].viewmatrix.data_ptr(), radii.data_ptr(), mp["pos"][v].data_ptr(), gs[v].data_ptr(), dz.data_ptr(),
                                       means3D.grad.data_ptr())

    def _pooled(self, c: _Call, cap: int) -> dict:
        """The batch's buffers, one tensor per kind for all views, and its tgs_view_t array: kept while the shapes and the capacity stay.
        ``c.names`` (of "alpha", "depth", "features"): the extra maps asked for -- their buffers [V,1,H,W], the depth's dz scratch [V, cap] and
        the tgs_view_extras_t array exist only then, and a call without them keeps the key (and the pool) it always had.  ``c.Cf`` > 0 (with
        "features" in ``c.names``): the feature map's buffer [V,Cf,H,W] and the tgs_view_features_t array; the feature scratch [V, cap * Cf]
        comes with the first feature gradient (_set_extra_grads)."""
        dev, names, Cf = c.params["means3D"].device, c.names, c.Cf
        key = (c.P, c.H, c.W, c.V, c.M, cap, dev, c.precomp) + ((tuple(names),) if names else ()) + ((Cf,) if Cf else ())
        if self._pool is None or self._pool["key"] != key:
            V, P = c.V, c.P
            gb, bb, ib = _C.state_sizes(P, c.W, c.H, not c.precomp, True, cap)
            al = lambda n: (n + 255) // 256 * 256
            z = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
            self._pool = dict(key=key, images=z(V, 3, c.H, c.W), radii=z(V, P, dt=torch.int32), g2d=z(V, P, 3), geom=z(V, al(gb), dt=torch.uint8),
                              binning=z(V, al(bb), dt=torch.uint8), img=z(V, al(ib), dt=torch.uint8), sizes=(gb, bb, ib), arr=_C.ViewArray(V),
                              gcol=z(V, P, 3) if c.precomp else None,
                              host=torch.empty((V, _C.META_BYTES), dtype=torch.uint8, pin_memory=True))
            xnames = [name for name in names if name != "features"]
            if Cf:
                self._pool.update(features=z(V, Cf, c.H, c.W), farr=_C.ViewFeaturesArray(V), fscratch=None, fscratch_shape=(V, cap * Cf))
            if xnames:
                self._pool.update({name: z(V, 1, c.H, c.W) for name in xnames}, xarr=_C.ViewExtrasArray(V))
                if "depth" in names:
                    self._pool["dz"] = z(V, cap)            # one float per instance slot and view (tgs_view_extras_t.dz_scratch)
        return self._pool

    def _fill_views(self, c: _Call, pool: dict) -> None:
        """The pooled tgs_view_t array: each view's camera, its slices of the pooled buffers and its grid bounds (dL_dpix comes later)."""
        gb, bb, ib = pool["sizes"]
        tcap = self.tile_capacity()
        # (generous: the class counts move more from view to view than the number of tiles with instances does, and a miss costs a frame)
        heavy, mid = ((int(self.class_bound[0] * 1.5) + 64) // 32 * 32, (int(self.class_bound[1] * 1.3) + 128) // 64 * 64) if tcap else (0, 0)
        for v, rs in enumerate(c.settings):
            a = pool["arr"][v]
            a.width, a.height, a.tan_fovx, a.tan_fovy = c.W, c.H, float(rs.tanfovx), float(rs.tanfovy)
            a.viewmatrix, a.projmatrix, a.campos, a.background = rs.viewmatrix.data_ptr(), rs.projmatrix.data_ptr(), rs.campos.data_ptr(), rs.bg.data_ptr()
            a.radii = a.radii_out = pool["radii"][v].data_ptr()
            a.geom_buffer, a.binning_buffer, a.img_buffer = pool["geom"][v].data_ptr(), pool["binning"][v].data_ptr(), pool["img"][v].data_ptr()
            a.geom_bytes, a.binning_bytes, a.img_bytes = gb, bb, ib
            a.out_color, a.dL_dmean2D, a.dL_dpix = pool["images"][v].data_ptr(), pool["g2d"][v].data_ptr(), None
            a.dL_dcolor = pool["gcol"][v].data_ptr() if c.precomp else None
            a.colors_precomp = c.colors[v].data_ptr() if c.precomp else None
            a.host_meta = pool["host"][v].data_ptr()        # k_scan writes the frame's Meta record here itself: no device-to-host copy in the stream
            a.tile_bound = tcap
            a.heavy_bound, a.mid_bound = heavy, mid
            if "xarr" in pool:                              # the maps' slices; the gradients come later (_set_extra_grads)
                x = pool["xarr"][v]
                x.out_alpha = pool["alpha"][v].data_ptr() if "alpha" in pool else None
                x.out_depth = pool["depth"][v].data_ptr() if "depth" in pool else None
                x.dL_dalpha = x.dL_ddepth = x.dz_scratch = None
            if "farr" in pool:                              # the model's features and the map's slice; the gradient comes later (_set_extra_grads)
                f = pool["farr"][v]
                f.C, f.features, f.out_features = c.Cf, c.features.data_ptr(), pool["features"][v].data_ptr()
                f.dL_dfeature_map = f.feature_scratch = None

    @staticmethod
    def _set_extra_grads(c: _Call, pool: dict, grads: Sequence[tuple]) -> tuple:
        """The views' upstream gradients of the extra maps -- ``grads``: per view (v, dL/d image, the extra gradients in the order of
        ``c.names``, any of them None) -- into the pooled tgs_view_extras_t and tgs_view_features_t arrays -> (a view has a depth gradient,
        a view has a feature gradient).  The feature scratch [V, cap * C] (C floats per instance slot and view) is allocated with the first
        feature gradient the pool sees."""
        with_depth = with_feat = False
        for v, _g, gs in grads:
            g = dict(zip(c.names, gs))
            gA, gD, gF = g.get("alpha"), g.get("depth"), g.get("features")
            if "xarr" in pool:
                x = pool["xarr"][v]
                x.dL_dalpha = gA.data_ptr() if gA is not None else None
                x.dL_ddepth = gD.data_ptr() if gD is not None else None
                x.dz_scratch = pool["dz"][v].data_ptr() if gD is not None else None
                with_depth |= gD is not None
            if "farr" in pool:
                f = pool["farr"][v]
                if gF is not None and pool["fscratch"] is None:
                    pool["fscratch"] = torch.empty(pool["fscratch_shape"], dtype=torch.float32, device=gF.device)
                f.dL_dfeature_map = gF.data_ptr() if gF is not None else None
                f.feature_scratch = pool["fscratch"][v].data_ptr() if gF is not None else None
                with_feat |= gF is not None
        return with_depth, with_feat

    @staticmethod
    def _map_of(c: _Call, name: str, state: tuple) -> torch.Tensor:
        """The alpha / depth map [1,H,W] or the feature map [C,H,W] of a view from _render_view (the synchronous frame's state)."""
        R, _color, _radii, geom, binning, img = state[:6]
        if name == "alpha":
            return _C.alpha_from_state(img, c.H, c.W)
        if name == "features":
            return _C.features_from_state(geom, binning, img, c.features, c.P, c.H, c.W, int(R))
        return _C.depth_from_state(geom, binning, img, c.P, c.H, c.W, int(R))

    def _render_view(self, c: _Call, v: int) -> tuple:
        """View v through the synchronous forward, buffers sized from the true count: (R, color, radii, geom, binning, img)."""
        rs, p, e = c.settings[v], c.params, torch.Tensor([])
        return _C.rasterize_gaussians(rs.bg, p["means3D"].detach(), c.colors[v] if c.precomp else e, p["opacities"].detach(), p["scales"].detach(),
                                      p["rotations"].detach(), rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, c.H, c.W,
                                      e if c.precomp else p["sh"].detach(), c.D, rs.campos, rs.prefiltered, rs.debug, pruning=self._pruning)

    def _backward_view(self, c: _Call, v: int, state: tuple, dL: torch.Tensor, gcol, scratch, extra: Sequence = ()) -> torch.Tensor:
        """The backward of a view from _render_view, in place: adds into the parameters' .grad (per-view colours: this view's alone, in gcol[v])
        and returns dL/d means2D.  The one-view kernel writes dL_dsh by rows: a level-major .grad gets it through the row-major ``scratch``.
        ``extra``: the view's upstream gradients [1,H,W] / [C,H,W] (or None) of the extra maps ``c.names``; with one of the feature map,
        dL/d features is added into ``c.fgrad`` (None: features that need no gradient -- it goes to a buffer of its own that is dropped, the
        through-alpha share still reaches the parameters)."""
        rs, p, e = c.settings[v], c.params, torch.Tensor([])
        R, _color, radii, geom, binning, img = state[:6]
        kw = {"grad_out_" + n: g for n, g in zip(c.names, extra) if g is not None}
        into = {name: t.grad for name, t in p.items()}
        if "grad_out_features" in kw:
            kw["features"] = c.features
            into["features"] = c.fgrad if c.fgrad is not None else torch.zeros_like(c.features)
        if c.precomp:
            gcol[v].zero_()
            into["colors_precomp"] = gcol[v]
        elif scratch is not None:
            scratch.zero_()
            into["sh"] = scratch
        g2 = _C.rasterize_gaussians_backward_accumulate(rs.bg, p["means3D"].detach(), radii, c.colors[v] if c.precomp else e, p["scales"].detach(),
                                                        p["rotations"].detach(), rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
                                                        dL, e if c.precomp else p["sh"].detach(), c.D, rs.campos, geom, R, binning, img, rs.debug, into,
                                                        deterministic=self._deterministic, **kw)
        if scratch is not None:
            p["sh"].grad.add_(scratch)
        return g2

    def run(self, views: Iterable[int], rasterize: Callable, upstream: Callable[[int, torch.Tensor], torch.Tensor]) -> List[torch.Tensor]:
        """Renders and back-propagates ``views``; returns their images.

        View k runs on stream k mod ``streams``: the forward of one view (binning: L2 atomics and HBM) shares the GPU with
        the render kernels of others (VALU bound), and every kernel's tail is filled by somebody else's work.  With
        ``deferred`` (default) a view's backward only runs its per-pixel half; the per-Gaussian half of all views is ONE
        pass at the end (``DeferredBackward``), so the streams never wait for each other.  Without it the backwards are
        chained by events, because each adds into the same gradient buffers.  The calling stream waits for everything
        before ``run`` returns."""
        views = list(views)
        images: List[torch.Tensor] = []
        metas: List[torch.Tensor] = []
        cap = self.capacity()
        if not views:
            return images
        main = torch.cuda.current_stream()
        lanes = _lanes(main, min(self.streams, len(views)) if cap is not None else 1)
        if len(lanes) > 1:
            _fork(lanes)                                    # whatever the caller enqueued before (e.g. zeroing the gradients)
        ready = None
        fwd_done = [None] * len(lanes)
        prev_bwd = None
        collector = DeferredBackward() if (self.deferred and cap is not None) else None
        last_on_lane = [None] * len(lanes)
        for k, v in enumerate(views):
            st = lanes[k % len(lanes)]
            with torch.cuda.stream(st):
                _collector.batch = collector                # picked up by rasterize_accumulate's forward
                try:
                    img, _radii, meta = rasterize(v, cap)
                finally:
                    _collector.batch = None
                metas.append(meta)
                if len(lanes) > 1:
                    fwd_done[k % len(lanes)] = torch.cuda.Event()
                    fwd_done[k % len(lanes)].record(st)
                if k == len(views) - 1:
                    # every Meta record is final once its forward has run: start the read-back NOW, in front of the last
                    # backward, so the host learns the verdict while the GPU is still busy
                    for i, ev in enumerate(fwd_done):
                        if ev is not None and lanes[i] is not st:
                            st.wait_event(ev)
                    for m in metas:
                        m.record_stream(st)
                    stacked = torch.stack(metas)
                    if self._host is None or self._host.shape != stacked.shape:
                        self._host = torch.empty(stacked.shape, dtype=torch.uint8, pin_memory=True)
                    self._host.copy_(stacked, non_blocking=True)
                    ready = torch.cuda.Event()
                    ready.record(st)
                grad = upstream(v, img.detach())
                if collector is None and prev_bwd is not None and len(lanes) > 1:
                    st.wait_event(prev_bwd)                 # gradient accumulation is read-modify-write: one backward at a time
                img.backward(grad)
                if len(lanes) > 1:
                    prev_bwd = torch.cuda.Event()
                    prev_bwd.record(st)
                    last_on_lane[k % len(lanes)] = prev_bwd
                    if st is not main:
                        img.record_stream(main)
            images.append(img.detach())
        if len(lanes) > 1:
            for ev in (last_on_lane if collector is not None else [prev_bwd]):
                if ev is not None:
                    main.wait_event(ev)                     # chained backwards: the last one is behind every other kernel of the batch
        if collector is not None:
            collector.finish()                              # the per-Gaussian half of every view, one pass, on the calling stream
        rows = _read_verdicts([ready], self._host)          # the one host wait of the batch
        seen = 0
        for i, (v, (R, rejected, _tiles)) in enumerate(zip(views, rows)):
            if rejected:
                self.rejected += 1
                img, _radii, meta = rasterize(v, None)      # synchronous forward: sizes its buffers from the true count
                img.backward(upstream(v, img.detach()))
                images[i] = img.detach()
                R, _ = _C.decode_meta(meta)
            seen = max(seen, R)
        self._learn(seen)
        return images
