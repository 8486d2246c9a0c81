"""The mesh rasterizer with gradients: ``import youreditableavatar_amd.mesh_raster_grad as dr`` serves ``tetgs_spatial/utils/rasterize.py`` with
that one import line changed.

The geometry stage trains through its rasterizer (``models/renderers/part_nvdiff_rasterizer.py`` :101-198, ``models/geometry/implicit_sdf.py``
:266-317): ``rasterize``, ``interpolate`` and ``antialias`` are autograd functions here.  Their forward is ``mesh_raster``'s / ``mesh_raster_aa``'s
native call, bit for bit; their backward is ``tgs_mesh_rasterize_backward`` / ``tgs_mesh_interpolate_backward`` / ``tgs_mesh_antialias_backward``
(csrc/tgs_mesh_grad.hip; the rules are written down in include/tgs_raster.h, "mesh rasterizer: gradients").  HIP device only.  Gradients are
float32 on the device; a backward launches nothing for an input that does not need a gradient; where ``pos`` or ``attr`` is shared by the N
images, the images' gradients are added in ascending image order.  Two runs give the same bits.

``RasterizeCudaContext``, ``face_ids``, ``hit_faces`` and ``antialias_construct_topology_hash`` are the older modules', unchanged;
``RasterizeGLContext`` is the same stateless handle under the name the wrapper's ``context_type="gl"`` asks for.

Not here: ``rast_db`` / ``grad_db`` / ``diff_attrs``, a gradient on z/w, near-plane clipping, ranged mode.  Every integer decision (coverage, the
winning triangle, the antialias pairs) is held fixed at the snapped coordinates.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _mesh, mesh_raster as _mr, mesh_raster_aa as _aa
from ._mesh import _lib
from .mesh_raster import RasterizeCudaContext, face_ids, hit_faces  # noqa: F401
from .mesh_raster_aa import antialias_construct_topology_hash  # noqa: F401


class RasterizeGLContext(RasterizeCudaContext):
    """The same stateless handle: ``dr.RasterizeGLContext(device=...)`` of a wrapper whose ``context_type`` says ``"gl"`` stays as it is."""


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, glctx, pos, tri, resolution, validate):
        ctx.call = _mesh.rasterize(pos.detach(), tri, resolution, validate)     # the forward-only module's checks; the backward reads their record
        rast = _mr._rasterize(ctx.call, pos.detach(), tri)
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    def backward(ctx, g_rast):
        pos, tri, rast = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        N, H, W, V, _, F = ctx.call[:6]
        d_pos = torch.empty((N, V, 4), dtype=torch.float32, device=ctx.call.dev)
        g, tri_c = g_rast.contiguous(), tri.contiguous()
        _mesh.run_images(_lib.tgs_mesh_rasterize_backward, ctx.call, _mesh.grad_workspace_bytes, pos, lambda n, p: (
            V, F, p, tri_c.data_ptr(), W, H, rast[n].data_ptr(), g[n].data_ptr(), d_pos[n].data_ptr()))
        return None, d_pos.reshape(pos.shape), None, None, None


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri):
        ctx.call = _mesh.interpolate(attr.detach(), rast.detach(), tri)
        out = _mr._interpolate(ctx.call, attr.detach(), rast.detach(), tri)
        ctx.save_for_backward(attr, rast, tri)
        return out

    @staticmethod
    def backward(ctx, g_out):
        attr, rast, tri = ctx.saved_tensors
        need_attr, need_rast = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_attr or need_rast):
            return None, None, None
        N, H, W, V, Cn, F, dev, _ = ctx.call
        d_attr = [torch.empty((V, Cn), dtype=torch.float32, device=dev) for _ in range(N)] if need_attr else None
        d_rast = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev) if need_rast else None
        if N * H * W:
            g, rast_c, tri_c = g_out.contiguous(), rast.contiguous(), tri.contiguous()
            _mesh.run_images(_lib.tgs_mesh_interpolate_backward, ctx.call, _mesh.grad_workspace_bytes, attr, lambda n, a: (
                V, F, Cn, a, tri_c.data_ptr(), H * W, rast_c[n].data_ptr(), g[n].data_ptr(), d_attr[n].data_ptr() if need_attr else None,
                d_rast[n].data_ptr() if need_rast else None))
        return _mesh.input_grad(ctx.call, d_attr, attr) if need_attr else None, d_rast, None


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, topology_hash, boost):
        ctx.call = _mesh.antialias(color.detach(), rast.detach(), pos.detach(), tri, topology_hash)
        out, topo = _aa._antialias(ctx.call, color.detach(), rast.detach(), pos.detach(), tri, topology_hash)      # (topo: the forward's, built at most once)
        ctx.save_for_backward(color, rast, pos, tri, topo)
        ctx.boost = float(boost)
        return out

    @staticmethod
    def backward(ctx, g_out):
        color, rast, pos, tri, topo = ctx.saved_tensors
        need_color, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not (need_color or need_pos):
            return None, None, None, None, None, None
        N, H, W, V, Cn, F, dev, _ = ctx.call
        d_color = torch.empty((N, H, W, Cn), dtype=torch.float32, device=dev) if need_color else None
        d_pos = [torch.empty((V, 4), dtype=torch.float32, device=dev) for _ in range(N)] if need_pos else None
        if N * H * W:
            g, color_c, rast_c, tri_c = g_out.contiguous(), color.contiguous(), rast.contiguous(), tri.contiguous()
            _mesh.run_images(_lib.tgs_mesh_antialias_backward, ctx.call, _mesh.grad_workspace_bytes, pos, lambda n, p: (
                V, F, Cn, p, tri_c.data_ptr(), topo.data_ptr(), W, H, rast_c[n].data_ptr(), color_c[n].data_ptr(), g[n].data_ptr(),
                d_color[n].data_ptr() if need_color else None, d_pos[n].data_ptr() if need_pos else None, ctx.boost))
        return d_color, None, _mesh.input_grad(ctx.call, d_pos, pos) if need_pos else None, None, None, None


def _plain(t):
    """the tensor without its autograd history (for the forward-only modules, which refuse one that requires a gradient)"""
    return t.detach() if isinstance(t, torch.Tensor) and t.requires_grad else t


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and all(isinstance(t, torch.Tensor) for t in tensors) and any(t.requires_grad for t in tensors)


def rasterize(glctx, pos: torch.Tensor, tri: torch.Tensor, resolution: Sequence[int], grad_db: bool = True, validate: bool = True) -> Tuple[torch.Tensor, None]:
    """``mesh_raster.rasterize`` with a gradient: the same native forward call, so ``rast`` [N,H,W,4] has the same bits.
    ``rast`` is differentiable with respect to ``pos`` through its u and v channels only: the gradient that arrives on z/w and on the ID
    channel is ignored (as in the third-party rasterizer), and the z column of ``pos.grad`` is zero.  ``grad_db`` is accepted and ignored:
    there is no derivative output, the second result stays ``None``."""
    if not _wants_grad(pos):
        return _mr.rasterize(glctx, _plain(pos), tri, resolution, validate=validate)
    return _Rasterize.apply(glctx, pos, tri, resolution, validate), None


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, rast_db=None, diff_attrs=None) -> Tuple[torch.Tensor, None]:
    """``mesh_raster.interpolate`` with gradients: the same native forward call.  Differentiable with respect to ``attr`` ([V,C] and [1,V,C]
    take the sum over the N images, [N,V,C] takes it per image) and with respect to ``rast`` (channels 0 and 1; channels 2 and 3 get exact
    zeros).  ``rast_db`` and ``diff_attrs`` must be ``None``: there are no attribute derivatives."""
    if rast_db is not None or diff_attrs is not None:
        raise RuntimeError("youreditableavatar_amd.mesh_raster_grad has no attribute derivatives: rast_db and diff_attrs must be None")
    if not _wants_grad(attr, rast):
        return _mr.interpolate(_plain(attr), _plain(rast), tri)
    return _Interpolate.apply(attr, rast, tri), None


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash: Optional[torch.Tensor] = None,
              pos_gradient_boost: float = 1.0) -> torch.Tensor:
    """``mesh_raster_aa.antialias`` with gradients: the same native forward calls.  Differentiable with respect to ``color`` and ``pos`` (the
    silhouette gradient: x, y and w of the two vertices of every blended pair's exit edge); ``rast`` gets no gradient from it.
    ``pos_gradient_boost`` multiplies the ``pos`` gradient."""
    if not (_wants_grad(color, rast, pos) and (color.requires_grad or pos.requires_grad)):
        return _aa.antialias(_plain(color), _plain(rast), _plain(pos), tri, topology_hash=topology_hash, pos_gradient_boost=pos_gradient_boost)
    return _Antialias.apply(color, rast, pos, tri, topology_hash, pos_gradient_boost)
