"""The mesh rasterizer of the painting stage: ``import youreditableavatar_amd.mesh_raster as dr`` serves ``tetgs_inpainter/mask_mesh_0822.py``.

``MeshModel.__init__`` opens ``dr.RasterizeCudaContext`` (:56) and every mask and normal image of the stage is ``dr.rasterize`` followed by
``dr.interpolate`` (``mask_mesh`` :94-134, ``prepare_mask_proj`` :183-188, ``get_concat_mask`` :350-364).  Both are here with the third-party
rasterizer's calling convention, forward only, on ``tgs_mesh_rasterize`` / ``tgs_mesh_interpolate`` (csrc/tgs_mesh.hip; the rasterization rule is
written down in include/tgs_raster.h).  HIP device only.

Not here: ``antialias`` (INTEGRATION.md 4j gives the edit per call site), gradients, ``rast_db`` (the second result is ``None``), ranged mode and
near-plane clipping.  An input that requires a gradient is refused, not detached.  The same calls with gradients are in ``mesh_raster_grad``.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _mesh
from ._mesh import MAX_FACES, MAX_RESOLUTION, _lib  # noqa: F401


class RasterizeCudaContext:
    """A stateless handle: it exists so that ``self.glctx = dr.RasterizeCudaContext(device=self.device)`` stays as it is."""

    def __init__(self, device=None):
        self.device = device


def _rasterize(call: _mesh.Call, pos: torch.Tensor, tri: torch.Tensor) -> torch.Tensor:
    """the native forward of a checked call (``mesh_raster_grad`` comes here with ``pos`` detached) -> ``rast``"""
    N, H, W, V, F, dev = call.N, call.H, call.W, call.V, call.F, call.dev
    if F == 0 or V == 0:
        return torch.zeros((N, H, W, 4), dtype=torch.float32, device=dev)
    rast = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    tri_c = tri.contiguous()
    _mesh.run_images(_lib.tgs_mesh_rasterize, call, lambda c: _lib.tgs_mesh_workspace_bytes(F, W, H), pos,
                     lambda n, p: (V, F, p, tri_c.data_ptr(), W, H, rast[n].data_ptr()))
    return rast


def rasterize(glctx, pos: torch.Tensor, tri: torch.Tensor, resolution: Sequence[int], validate: bool = True) -> Tuple[torch.Tensor, None]:
    """``pos`` [N,V,4] or [V,4] float32 clip space, ``tri`` [F,3] int32, ``resolution`` (H, W) -> (``rast`` [N,H,W,4] float32, None).
    ``rast`` holds (u, v, z/w, triangle_id + 1), all zero where nothing is hit; row 0 is the row at clip y = -1.  With ``validate`` an index
    outside [0, V) raises ValueError before anything is launched (one reduction and one read-back); without it such a triangle produces nothing."""
    return _rasterize(_mesh.rasterize(pos, tri, resolution, validate), pos, tri), None


def _interpolate(call: _mesh.Call, attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor) -> torch.Tensor:
    """the native forward of a checked call -> ``out``"""
    N, H, W, V, Cn, F = call[:6]
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=call.dev)
    if N * H * W:
        rast_c, tri_c = rast.contiguous(), tri.contiguous()
        _mesh.run_images(_lib.tgs_mesh_interpolate, call, None, attr, lambda n, a: (V, F, Cn, a, tri_c.data_ptr(), H * W, rast_c[n].data_ptr(), out[n].data_ptr()))
    return out


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor) -> Tuple[torch.Tensor, None]:
    """``attr`` [N,V,C], [1,V,C] or [V,C] float32 (any C >= 1), ``rast`` [N,H,W,4] of ``rasterize``, ``tri`` [F,3] int32 ->
    (``out`` [N,H,W,C], None): out = u a0 + v a1 + (1 - u - v) a2 with the vertices of triangle id - 1, exactly 0 where id = 0."""
    return _interpolate(_mesh.interpolate(attr, rast, tri), attr, rast, tri), None


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
