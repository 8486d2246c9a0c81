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

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import mesh_raster as _mr
from . import mesh_raster_aa as _aa
from .diff_gaussian_rasterization import _C as _rast_c
from .mesh_raster import RasterizeCudaContext, face_ids, hit_faces  # noqa: F401
from .mesh_raster_aa import antialias_construct_topology_hash  # noqa: F401

_lib = _rast_c._lib
_lib.tgs_mesh_grad_workspace_bytes.restype = C.c_size_t
_lib.tgs_mesh_grad_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int64]
_lib.tgs_mesh_interpolate_backward.restype = C.c_int
_lib.tgs_mesh_interpolate_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t]
_lib.tgs_mesh_rasterize_backward.restype = C.c_int
_lib.tgs_mesh_rasterize_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_mesh_antialias_backward.restype = C.c_int
_lib.tgs_mesh_antialias_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t]


class RasterizeGLContext(RasterizeCudaContext):
    """The same stateless handle: ``dr.RasterizeGLContext(device=...)`` of a wrapper whose ``context_type`` says ``"gl"`` stays as it is."""


def _workspace(V: int, Cn: int, n_pixels: int, dev) -> Tuple[torch.Tensor, int]:
    nbytes = int(_lib.tgs_mesh_grad_workspace_bytes(V, Cn, n_pixels))
    if nbytes == 0:
        raise RuntimeError(f"no gradient workspace for V = {V}, C = {Cn}, {n_pixels} pixels")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _sum_images(per_image, like: torch.Tensor) -> torch.Tensor:
    """the images' gradients of a shared input, added in ascending image order -> ``like``'s shape"""
    total = per_image[0]
    for g in per_image[1:]:
        total = total + g
    return total.reshape(like.shape)


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, glctx, pos, tri, resolution, validate):
        rast, _ = _mr.rasterize(glctx, pos.detach(), tri, resolution, validate=validate)
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    def backward(ctx, g_rast):
        pos, tri, rast = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        clip = pos if pos.dim() == 3 else pos[None]
        N, V, F = int(clip.shape[0]), int(clip.shape[1]), int(tri.shape[0])
        H, W = int(rast.shape[1]), int(rast.shape[2])
        dev = pos.device
        d_pos = torch.empty((N, V, 4), dtype=torch.float32, device=dev)
        g, tri_c = g_rast.contiguous(), tri.contiguous()
        with torch.cuda.device(dev):
            ws, nbytes = _workspace(V, 4, H * W, dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for n in range(N):
                p = clip[n].contiguous()
                r = _lib.tgs_mesh_rasterize_backward(st, V, F, p.data_ptr(), tri_c.data_ptr(), W, H, rast[n].data_ptr(), g[n].data_ptr(), d_pos[n].data_ptr(),
                                                     ws.data_ptr(), nbytes)
                if r < 0:
                    raise _rast_c._err(r)
        return None, d_pos.reshape(pos.shape), None, None, None


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri):
        out, _ = _mr.interpolate(attr.detach(), rast.detach(), tri)
        ctx.save_for_backward(attr, rast, tri)
        return out

    @staticmethod
    def backward(ctx, g_out):
        attr, rast, tri = ctx.saved_tensors
        need_attr, need_rast = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_attr or need_rast):
            return None, None, None
        N, H, W = (int(x) for x in rast.shape[:3])
        V, Cn, F = int(attr.shape[-2]), int(attr.shape[-1]), int(tri.shape[0])
        dev = rast.device
        per_image = attr.dim() == 3 and attr.shape[0] == N and N != 1
        d_attr = [torch.empty((V, Cn), dtype=torch.float32, device=dev) for _ in range(N)] if need_attr else None
        d_rast = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev) if need_rast else None
        if N * H * W:
            g, rast_c, tri_c = g_out.contiguous(), rast.contiguous(), tri.contiguous()
            with torch.cuda.device(dev):
                ws, nbytes = _workspace(V, Cn, H * W, dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                for n in range(N):
                    a = (attr if attr.dim() == 2 else attr[n if attr.shape[0] == N else 0]).contiguous()
                    r = _lib.tgs_mesh_interpolate_backward(st, V, F, Cn, a.data_ptr(), tri_c.data_ptr(), H * W, rast_c[n].data_ptr(), g[n].data_ptr(),
                                                           _ptr(d_attr[n]) if need_attr else None, _ptr(d_rast[n]) if need_rast else None, ws.data_ptr(), nbytes)
                    if r < 0:
                        raise _rast_c._err(r)
        g_attr = None
        if need_attr:
            g_attr = torch.zeros_like(attr) if not N * H * W else torch.stack(d_attr) if per_image else _sum_images(d_attr, attr)
        return g_attr, d_rast, None


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, topo, boost):
        out = _aa.antialias(color.detach(), rast.detach(), pos.detach(), tri, topology_hash=topo, pos_gradient_boost=boost)
        ctx.save_for_backward(color, rast, pos, tri, topo)
        ctx.boost = float(boost)
        return out

    @staticmethod
    def backward(ctx, g_out):
        color, rast, pos, tri, topo = ctx.saved_tensors
        need_color, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not (need_color or need_pos):
            return None, None, None, None, None, None
        N, H, W = (int(x) for x in rast.shape[:3])
        V, Cn, F = int(pos.shape[-2]), int(color.shape[-1]), int(tri.shape[0])
        dev = color.device
        per_image = pos.dim() == 3 and pos.shape[0] == N and N != 1
        d_color = torch.empty((N, H, W, Cn), dtype=torch.float32, device=dev) if need_color else None
        d_pos = [torch.empty((V, 4), dtype=torch.float32, device=dev) for _ in range(N)] if need_pos else None
        if N * H * W:
            g, color_c, rast_c, tri_c, topo_c = g_out.contiguous(), color.contiguous(), rast.contiguous(), tri.contiguous(), topo.contiguous()
            with torch.cuda.device(dev):
                ws, nbytes = _workspace(V, Cn, H * W, dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                for n in range(N):
                    p = (pos if pos.dim() == 2 else pos[n if pos.shape[0] == N else 0]).contiguous()
                    r = _lib.tgs_mesh_antialias_backward(st, V, F, Cn, p.data_ptr(), tri_c.data_ptr(), topo_c.data_ptr(), W, H, rast_c[n].data_ptr(), color_c[n].data_ptr(),
                                                         g[n].data_ptr(), _ptr(d_color[n]) if need_color else None, _ptr(d_pos[n]) if need_pos else None, ctx.boost,
                                                         ws.data_ptr(), nbytes)
                    if r < 0:
                        raise _rast_c._err(r)
        g_pos = None
        if need_pos:
            g_pos = torch.zeros_like(pos) if not N * H * W else torch.stack(d_pos) if per_image else _sum_images(d_pos, pos)
        return d_color, None, g_pos, None, None, None


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


def _shared_topology(tri, pos) -> torch.Tensor:
    """The topology the forward and the backward of one ``antialias`` call share, built once.  Where ``tri`` or ``pos`` is not what the forward
    accepts (or names no triangle), an empty table: the forward's own checks speak, in their order."""
    usable = isinstance(tri, torch.Tensor) and tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3 and tri.shape[0] <= _mr.MAX_FACES
    F = int(tri.shape[0]) if usable else 0
    V = int(pos.shape[-2]) if pos.dim() >= 2 else 0
    if usable and tri.is_cuda and F and V:
        return _aa._topology(tri, V)
    return torch.empty((F, 3), dtype=torch.int32, device=tri.device if usable else None)


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash: Optional[torch.Tensor] = None,
              pos_gradient_boost: float = 1.0) -> torch.Tensor:
    """``mesh_raster_aa.antialias`` with gradients: the same native forward calls.  Differentiable with respect to ``color`` and ``pos`` (the
    silhouette gradient: x, y and w of the two vertices of every blended pair's exit edge); ``rast`` gets no gradient from it.
    ``pos_gradient_boost`` multiplies the ``pos`` gradient."""
    if not (_wants_grad(color, rast, pos) and (color.requires_grad or pos.requires_grad)):
        return _aa.antialias(_plain(color), _plain(rast), _plain(pos), tri, topology_hash=topology_hash, pos_gradient_boost=pos_gradient_boost)
    topo = topology_hash if topology_hash is not None else _shared_topology(tri, pos)
    return _Antialias.apply(color, rast, pos, tri, topo, pos_gradient_boost)
