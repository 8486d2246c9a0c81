"""The mesh rasterizer with ``antialias``: ``import youreditableavatar_amd.mesh_raster_aa as dr`` serves ``tetgs_inpainter/mask_mesh_0822.py``
without call-site edits.

``RasterizeCudaContext``, ``rasterize``, ``interpolate``, ``face_ids`` and ``hit_faces`` are ``mesh_raster``'s, unchanged.  Added here are
``antialias`` (:98, :139-141, :188, :356, :364 of that file; ``part_nvdiff_rasterizer.py`` :108-191) and
``antialias_construct_topology_hash``, on ``tgs_mesh_antialias`` / ``tgs_mesh_topology`` (csrc/tgs_mesh_aa.hip; the rule is written down in
include/tgs_raster.h, "mesh rasterizer: antialias").  HIP device only, forward only: an input that requires a gradient is refused, not detached.

Not here: gradients (``pos_gradient_boost`` is accepted and ignored), ``rast_db``, near-plane clipping.  The same calls with gradients are in
``mesh_raster_grad``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _mesh
from ._mesh import _lib
from .mesh_raster import RasterizeCudaContext, face_ids, hit_faces, interpolate, rasterize  # noqa: F401


def antialias_construct_topology_hash(tri: torch.Tensor, num_vertices: Optional[int] = None) -> torch.Tensor:
    """``tri`` [F,3] int32 -> int32 [F,3] on ``tri``'s device: per edge k (vertex k to vertex k+1) -1 if no other triangle has it, the other
    triangle's opposite vertex if exactly one has it, -2 if more than one.  Built once per mesh and passed to ``antialias`` as
    ``topology_hash``.  A triangle with a repeated index, a negative one or (with ``num_vertices``) one >= num_vertices has -1 in its row and
    is nobody's neighbour."""
    call = _mesh.topology(tri, num_vertices)
    return _mesh.build_topology(tri, call.V, call.F, call.dev)


def _antialias(call: _mesh.Call, color, rast, pos, tri, topology_hash) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """the native forward of a checked call -> ``out`` and the topology it worked with (``None`` where there was no pixel to work on)"""
    N, H, W, V, Cn, F = call[:6]
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=call.dev)
    if not N * H * W:
        return out, None
    topo = _mesh.topology_of(call, tri, topology_hash)
    color_c, rast_c, tri_c = color.contiguous(), rast.contiguous(), tri.contiguous()
    _mesh.run_images(_lib.tgs_mesh_antialias, call, lambda c: _lib.tgs_mesh_antialias_workspace_bytes(W, H), pos, lambda n, p: (
        V, F, Cn, p, tri_c.data_ptr(), topo.data_ptr(), W, H, rast_c[n].data_ptr(), color_c[n].data_ptr(), out[n].data_ptr()))
    return out, topo


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash: Optional[torch.Tensor] = None,
              pos_gradient_boost: float = 1.0) -> torch.Tensor:
    """``color`` [N,H,W,C] float32 (any C >= 1), ``rast`` [N,H,W,4] of ``rasterize``, ``pos`` [N,V,4], [1,V,4] or [V,4] float32, ``tri`` [F,3]
    int32 -> ``out`` [N,H,W,C] (the tensor itself, not a tuple): ``color`` blended across silhouette edges between horizontally and vertically
    adjacent pixels.  ``topology_hash`` is what ``antialias_construct_topology_hash(tri)`` returned; ``None`` builds it in the call.
    ``pos_gradient_boost`` is accepted and ignored (forward only)."""
    return _antialias(_mesh.antialias(color, rast, pos, tri, topology_hash), color, rast, pos, tri, topology_hash)[0]
