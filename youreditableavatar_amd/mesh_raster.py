"""The mesh rasterizer of the painting stage: ``import youreditableavatar_amd.mesh_raster as dr`` serves ``tetgs_inpainter/mask_mesh_0822.py``.

``MeshModel.__init__`` opens ``dr.RasterizeCudaContext`` (:56) and every mask and normal image of the stage is ``dr.rasterize`` followed by
``dr.interpolate`` (``mask_mesh`` :94-134, ``prepare_mask_proj`` :183-188, ``get_concat_mask`` :350-364).  Both are here with the third-party
rasterizer's calling convention, forward only, on ``tgs_mesh_rasterize`` / ``tgs_mesh_interpolate`` (csrc/tgs_mesh.hip; the rasterization rule is
written down in include/tgs_raster.h).  HIP device only.

Not here: ``antialias`` (INTEGRATION.md 4j gives the edit per call site), gradients, ``rast_db`` (the second result is ``None``), ranged mode and
near-plane clipping.  An input that requires a gradient is refused, not detached.  The same calls with gradients are in ``mesh_raster_grad``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .diff_gaussian_rasterization import _C as _rast_c

_lib = _rast_c._lib
_lib.tgs_mesh_workspace_bytes.restype = C.c_size_t
_lib.tgs_mesh_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
_lib.tgs_mesh_rasterize.restype = C.c_int
_lib.tgs_mesh_rasterize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_mesh_interpolate.restype = C.c_int
_lib.tgs_mesh_interpolate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]

MAX_FACES = (1 << 24) - 1          # the triangle ID travels in a float
MAX_RESOLUTION = 8192


class RasterizeCudaContext:
    """A stateless handle: it exists so that ``self.glctx = dr.RasterizeCudaContext(device=self.device)`` stays as it is."""

    def __init__(self, device=None):
        self.device = device


def _refuse_grad(name: str, t: torch.Tensor) -> None:
    if t.requires_grad:
        raise RuntimeError(f"youreditableavatar_amd.mesh_raster is forward only: `{name}` requires a gradient and none would flow (pass {name}.detach() if that is intended)")


def _need_device(**tensors) -> None:
    """checked last, behind everything that can be said about the arguments without a device"""
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"youreditableavatar_amd.mesh_raster has no CPU path: {name} must be on a HIP device")
    devs = {t.device for t in tensors.values()}
    if len(devs) != 1:
        raise RuntimeError("all tensors must be on one device, got " + ", ".join(f"{n} on {t.device}" for n, t in tensors.items()))


def _check_tri(tri: torch.Tensor) -> None:
    if not isinstance(tri, torch.Tensor):
        raise RuntimeError("tri must be a tensor")
    if tri.dtype != torch.int32 or tri.dim() != 2 or tri.shape[1] != 3:
        raise RuntimeError(f"expected int32 tri of shape [F,3], got {tri.dtype} {tuple(tri.shape)}")
    if tri.shape[0] > MAX_FACES:
        raise RuntimeError(f"tri has {tri.shape[0]} faces; at most 2^24 - 1 = {MAX_FACES} (the triangle ID is carried in a float)")


def rasterize(glctx, pos: torch.Tensor, tri: torch.Tensor, resolution: Sequence[int], validate: bool = True) -> Tuple[torch.Tensor, None]:
    """``pos`` [N,V,4] or [V,4] float32 clip space, ``tri`` [F,3] int32, ``resolution`` (H, W) -> (``rast`` [N,H,W,4] float32, None).
    ``rast`` holds (u, v, z/w, triangle_id + 1), all zero where nothing is hit; row 0 is the row at clip y = -1.  With ``validate`` an index
    outside [0, V) raises ValueError before anything is launched (one reduction and one read-back); without it such a triangle produces nothing."""
    if not isinstance(pos, torch.Tensor):
        raise RuntimeError("pos must be a tensor")
    if pos.dtype != torch.float32 or pos.dim() not in (2, 3) or pos.shape[-1] != 4:
        raise RuntimeError(f"expected float32 pos of shape [N,V,4] or [V,4], got {pos.dtype} {tuple(pos.shape)}")
    _check_tri(tri)
    _refuse_grad("pos", pos)
    H, W = (int(resolution[0]), int(resolution[1])) if len(resolution) == 2 else (0, 0)
    if not (0 < H <= MAX_RESOLUTION and 0 < W <= MAX_RESOLUTION):
        raise RuntimeError(f"resolution must be (H, W) with 1 <= H, W <= {MAX_RESOLUTION}, got {tuple(resolution)}")
    clip = pos if pos.dim() == 3 else pos[None]
    N, V, F = int(clip.shape[0]), int(clip.shape[1]), int(tri.shape[0])
    if validate and F:
        lo, hi = (int(x) for x in torch.aminmax(tri))
        if lo < 0 or hi >= V:
            raise ValueError(f"tri holds vertex indices in [{lo}, {hi}]; pos has {V} vertices")
    _need_device(pos=pos, tri=tri)
    dev = pos.device
    if F == 0 or V == 0:
        return torch.zeros((N, H, W, 4), dtype=torch.float32, device=dev), None
    rast = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    tri_c = tri.contiguous()
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_mesh_workspace_bytes(F, W, H))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for n in range(N):
            p = clip[n].contiguous()
            r = _lib.tgs_mesh_rasterize(st, V, F, p.data_ptr(), tri_c.data_ptr(), W, H, rast[n].data_ptr(), ws.data_ptr(), nbytes)
            if r < 0:
                raise _rast_c._err(r)
    return rast, None


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor) -> Tuple[torch.Tensor, None]:
    """``attr`` [N,V,C], [1,V,C] or [V,C] float32 (any C >= 1), ``rast`` [N,H,W,4] of ``rasterize``, ``tri`` [F,3] int32 ->
    (``out`` [N,H,W,C], None): out = u a0 + v a1 + (1 - u - v) a2 with the vertices of triangle id - 1, exactly 0 where id = 0."""
    if not isinstance(attr, torch.Tensor) or not isinstance(rast, torch.Tensor):
        raise RuntimeError("attr and rast must be tensors")
    if rast.dtype != torch.float32 or rast.dim() != 4 or rast.shape[-1] != 4:
        raise RuntimeError(f"expected float32 rast of shape [N,H,W,4], got {rast.dtype} {tuple(rast.shape)}")
    N, H, W = (int(x) for x in rast.shape[:3])
    if attr.dtype != torch.float32 or attr.dim() not in (2, 3) or attr.shape[-1] < 1 or (attr.dim() == 3 and attr.shape[0] not in (1, N)):
        raise RuntimeError(f"expected float32 attr of shape [{N},V,C], [1,V,C] or [V,C] with C >= 1, got {attr.dtype} {tuple(attr.shape)}")
    _check_tri(tri)
    _refuse_grad("attr", attr)
    _refuse_grad("rast", rast)
    _need_device(attr=attr, rast=rast, tri=tri)
    V, Cn, F = int(attr.shape[-2]), int(attr.shape[-1]), int(tri.shape[0])
    dev = rast.device
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=dev)
    if N * H * W == 0:
        return out, None
    rast_c, tri_c = rast.contiguous(), tri.contiguous()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        for n in range(N):
            a = (attr if attr.dim() == 2 else attr[n if attr.shape[0] == N else 0]).contiguous()
            r = _lib.tgs_mesh_interpolate(st, V, F, Cn, a.data_ptr(), tri_c.data_ptr(), H * W, rast_c[n].data_ptr(), out[n].data_ptr())
            if r < 0:
                raise _rast_c._err(r)
    return out, None


def face_ids(rast: torch.Tensor) -> torch.Tensor:
    """``rast`` [N,H,W,4] -> int32 [N,H,W]: the triangle index of every pixel, -1 where nothing is hit."""
    if rast.dim() != 4 or rast.shape[-1] != 4:
        raise RuntimeError(f"expected rast of shape [N,H,W,4], got {tuple(rast.shape)}")
    return rast[..., 3].to(torch.int32) - 1


def hit_faces(rast: torch.Tensor, mask: torch.Tensor, num_faces: Optional[int] = None) -> torch.Tensor:
    """The faces visible under a 2-D mask: ``rast`` [1,H,W,4] (or one image [H,W,4]), ``mask`` [H,W] (nonzero = selected) -> bool [F].
    What ``back_project`` takes from ray casting (mask_mesh_0822.py): the triangles hit by the rays through the selected pixels.  ``num_faces``
    is F; without it the result ends at the largest ID in ``rast`` (one read-back)."""
    img = rast if rast.dim() == 3 else rast[0]
    if rast.dim() == 4 and rast.shape[0] != 1:
        raise RuntimeError("hit_faces takes one image: rast [1,H,W,4] or [H,W,4]")
    if mask.dim() != 2 or tuple(mask.shape) != tuple(img.shape[:2]):
        raise RuntimeError(f"expected a mask of shape {tuple(img.shape[:2])}, got {tuple(mask.shape)}")
    ids = face_ids(img[None])[0].to(torch.int64)
    n = int(num_faces) if num_faces is not None else (int(ids.max()) + 1 if ids.numel() else 0)
    sel = ids[(mask.to(ids.device) != 0) & (ids >= 0)]
    out = torch.zeros(n, dtype=torch.bool, device=ids.device)
    out[sel] = True
    return out
