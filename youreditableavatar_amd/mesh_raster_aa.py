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

import ctypes as C
from typing import Optional

import torch

from .diff_gaussian_rasterization import _C as _rast_c
from .mesh_raster import (MAX_RESOLUTION, RasterizeCudaContext, _check_tri, _need_device, _refuse_grad, face_ids, hit_faces, interpolate,  # noqa: F401
                          rasterize)

_lib = _rast_c._lib
_lib.tgs_mesh_topology_workspace_bytes.restype = C.c_size_t
_lib.tgs_mesh_topology_workspace_bytes.argtypes = [C.c_int]
_lib.tgs_mesh_topology.restype = C.c_int
_lib.tgs_mesh_topology.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_mesh_antialias_workspace_bytes.restype = C.c_size_t
_lib.tgs_mesh_antialias_workspace_bytes.argtypes = [C.c_int, C.c_int]
_lib.tgs_mesh_antialias.restype = C.c_int
_lib.tgs_mesh_antialias.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t]

_ANY_VERTEX = (1 << 31) - 1        # num_vertices when only tri is known: every non-negative index names a vertex


def _topology(tri: torch.Tensor, V: int) -> torch.Tensor:
    """tri already checked and on a device -> int32 [F,3]"""
    F, dev = int(tri.shape[0]), tri.device
    topo = torch.empty((F, 3), dtype=torch.int32, device=dev)
    if F == 0:
        return topo
    tri_c = tri.contiguous()
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_mesh_topology_workspace_bytes(F))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        r = _lib.tgs_mesh_topology(torch.cuda.current_stream(dev).cuda_stream, V, F, tri_c.data_ptr(), topo.data_ptr(), ws.data_ptr(), nbytes)
        if r < 0:
            raise _rast_c._err(r)
    return topo


def antialias_construct_topology_hash(tri: torch.Tensor, num_vertices: Optional[int] = None) -> torch.Tensor:
    """``tri`` [F,3] int32 -> int32 [F,3] on ``tri``'s device: per edge k (vertex k to vertex k+1) -1 if no other triangle has it, the other
    triangle's opposite vertex if exactly one has it, -2 if more than one.  Built once per mesh and passed to ``antialias`` as
    ``topology_hash``.  A triangle with a repeated index, a negative one or (with ``num_vertices``) one >= num_vertices has -1 in its row and
    is nobody's neighbour."""
    _check_tri(tri)
    V = _ANY_VERTEX if num_vertices is None else int(num_vertices)
    if V < 0:
        raise RuntimeError(f"num_vertices must be >= 0, got {num_vertices}")
    _need_device(tri=tri)
    return _topology(tri, V)


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash: Optional[torch.Tensor] = None,
              pos_gradient_boost: float = 1.0) -> torch.Tensor:
    """``color`` [N,H,W,C] float32 (any C >= 1), ``rast`` [N,H,W,4] of ``rasterize``, ``pos`` [N,V,4], [1,V,4] or [V,4] float32, ``tri`` [F,3]
    int32 -> ``out`` [N,H,W,C] (the tensor itself, not a tuple): ``color`` blended across silhouette edges between horizontally and vertically
    adjacent pixels.  ``topology_hash`` is what ``antialias_construct_topology_hash(tri)`` returned; ``None`` builds it in the call.
    ``pos_gradient_boost`` is accepted and ignored (forward only)."""
    if not isinstance(color, torch.Tensor) or not isinstance(rast, torch.Tensor) or not isinstance(pos, torch.Tensor):
        raise RuntimeError("color, rast and pos must be tensors")
    if rast.dtype != torch.float32 or rast.dim() != 4 or rast.shape[-1] != 4:
        raise RuntimeError(f"expected float32 rast of shape [N,H,W,4], got {rast.dtype} {tuple(rast.shape)}")
    N, H, W = (int(x) for x in rast.shape[:3])
    if color.dtype != torch.float32 or color.dim() != 4 or tuple(color.shape[:3]) != (N, H, W) or color.shape[-1] < 1:
        raise RuntimeError(f"expected float32 color of shape [{N},{H},{W},C] with C >= 1, got {color.dtype} {tuple(color.shape)}")
    if pos.dtype != torch.float32 or pos.dim() not in (2, 3) or pos.shape[-1] != 4 or (pos.dim() == 3 and pos.shape[0] not in (1, N)):
        raise RuntimeError(f"expected float32 pos of shape [{N},V,4], [1,V,4] or [V,4], got {pos.dtype} {tuple(pos.shape)}")
    _check_tri(tri)
    if N * H * W and not (H <= MAX_RESOLUTION and W <= MAX_RESOLUTION):
        raise RuntimeError(f"rast must have 1 <= H, W <= {MAX_RESOLUTION}, got {tuple(rast.shape)}")
    V, Cn, F = int(pos.shape[-2]), int(color.shape[-1]), int(tri.shape[0])
    if topology_hash is not None:
        if not isinstance(topology_hash, torch.Tensor) or topology_hash.dtype != torch.int32 or tuple(topology_hash.shape) != (F, 3):
            got = f"{topology_hash.dtype} {tuple(topology_hash.shape)}" if isinstance(topology_hash, torch.Tensor) else type(topology_hash).__name__
            raise RuntimeError(f"expected the int32 [{F},3] topology of antialias_construct_topology_hash(tri) as topology_hash, got {got}")
    for name, t in (("color", color), ("rast", rast), ("pos", pos)):
        _refuse_grad(name, t)
    _need_device(color=color, rast=rast, pos=pos, tri=tri)
    dev = color.device
    if topology_hash is not None and topology_hash.device != dev:
        raise RuntimeError(f"topology_hash is on {topology_hash.device}, tri on {dev}: the topology is built on tri's device")
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=dev)
    if N * H * W == 0:
        return out
    if topology_hash is not None:
        topo = topology_hash.contiguous()
    else:
        topo = _topology(tri, V) if F and V else torch.empty((F, 3), dtype=torch.int32, device=dev)     # (no faces or no vertices: the call copies)
    color_c, rast_c, tri_c = color.contiguous(), rast.contiguous(), tri.contiguous()
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_mesh_antialias_workspace_bytes(W, H))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for n in range(N):
            p = (pos if pos.dim() == 2 else pos[n if pos.shape[0] == N else 0]).contiguous()
            r = _lib.tgs_mesh_antialias(st, V, F, Cn, p.data_ptr(), tri_c.data_ptr(), topo.data_ptr(), W, H, rast_c[n].data_ptr(), color_c[n].data_ptr(),
                                        out[n].data_ptr(), ws.data_ptr(), nbytes)
            if r < 0:
                raise _rast_c._err(r)
    return out
