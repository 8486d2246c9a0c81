"""Rays against a triangle mesh: the first operation of the editing pipeline, with the call shape of ``o3d.t.geometry.RaycastingScene``.

``mesh_localization.py`` (:150-167, :89-131) and ``back_project`` of ``tetgs_inpainter/mask_mesh_0822.py`` (:209-237) build an open3d scene per camera, call
``scene.cast_rays(rays)`` and put the ``primitive_ids`` into a Python set, one ``add`` per ray.  ``RaycastingScene`` here answers a numpy array with numpy
arrays, so those lines keep their shape (the ``.numpy()`` of open3d's tensors goes), and answers a float32 device tensor with device tensors on the current stream with no host read-back;
``hit_faces(rays)`` is the set itself, a ``bool[F]`` on the device that ``mesh_region.refine_region`` takes as it is.  The kernels are
``csrc/tgs_mesh_rays.hip``; the rules are written down in include/tgs_raster.h, "mesh ray casting", and restated in tests/mesh_rays_ref.py.  The tree is the one
``mesh_sdf.SDF`` builds on the host, once per mesh, and ``from_sdf`` shares it; the queries run on a HIP device only: there is no CPU path.  No autograd.

What differs from embree behind open3d (which nobody could run next to this; by its documentation): the arithmetic is in double; among hits of equal ``t``
the lowest face index is returned; ``t >= 0`` is inclusive, so an origin on a face hits it at 0; zero-area faces never hit; one mesh per scene.
``count_intersections``, ``list_intersections``, ``compute_closest_points`` and the distance and occupancy queries are not served and raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _host
from ._host import _F, _I, _L, _P, _Z, guard as _guard, need_device as _need_device, ok as _ok, raw_stream as _raw_stream
from . import mesh_sdf as _mesh_sdf

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h and tgs_mesh_rays_testing.h declare them (every pointer is a c_void_p)
    "tgs_meshrays_cast": (_I, [_P, _P, _Z, _I, _I, _P, _P, _I, _L, _P, _I, _P, _P, _P, _P, _P, _P]),
    "tgs_meshrays_occluded": (_I, [_P, _P, _Z, _I, _I, _P, _P, _I, _L, _P, _F, _F, _I, _P]),
    "tgs_meshrays_cast_host": (_I, [_P, _Z, _I, _I, _P, _P, _I, _L, _P, _I, _P, _P, _P, _P, _P, _P]),
    "tgs_meshrays_occluded_host": (_I, [_P, _Z, _I, _I, _P, _P, _I, _L, _P, _F, _F, _I, _P]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
_NOT_SERVED = ("youreditableavatar_amd.mesh_rays.RaycastingScene does not serve {}: it serves add_triangles, cast_rays, test_occlusions and hit_faces; "
               "mesh_sdf.SDF.closest gives the closest point and the distance")
_KEYS = ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals")


class RaycastingScene:
    """``RaycastingScene()`` then ``add_triangles(vertices, faces)``, or ``RaycastingScene(vertices, faces)``, or ``RaycastingScene.from_sdf(sdf)``.  The mesh is
    what ``mesh_sdf.SDF`` takes: ``vertices`` [V,3] floats, all finite, ``faces`` [F,3] integer indices in ``[0, V)``; numpy arrays or tensors on any device
    (read as float32 and int32).  One mesh per scene.  Without a HIP device the scene is built and every query raises."""

    INVALID_ID = 4294967295

    def __init__(self, vertices=None, faces=None):
        self._sdf = None
        if (vertices is None) != (faces is None):
            raise RuntimeError("RaycastingScene(vertices, faces) takes both or neither")
        if vertices is not None:
            self.add_triangles(vertices, faces)

    @classmethod
    def from_sdf(cls, sdf: "_mesh_sdf.SDF") -> "RaycastingScene":
        """the scene of an existing ``mesh_sdf.SDF``: its device arrays and its tree, without a second build"""
        if not isinstance(sdf, _mesh_sdf.SDF):
            raise RuntimeError(f"from_sdf takes a youreditableavatar_amd.mesh_sdf.SDF, got {type(sdf).__name__}")
        scene = cls()
        scene._sdf = sdf
        return scene

    def add_triangles(self, vertices, faces) -> int:
        """-> 0, the geometry id of the one mesh.  A second call raises: only one mesh per scene is served (concatenate the meshes instead)."""
        if self._sdf is not None:
            raise RuntimeError("youreditableavatar_amd.mesh_rays.RaycastingScene serves one mesh per scene, and this scene has its mesh: concatenate the meshes, or use a second scene")
        self._sdf = _mesh_sdf.SDF(vertices, faces)
        return 0

    device = property(lambda self: None if self._sdf is None else self._sdf.device)
    num_faces = property(lambda self: 0 if self._sdf is None else len(self._sdf.faces))

    def __repr__(self):
        return "RaycastingScene(empty)" if self._sdf is None else f"RaycastingScene(V={len(self._sdf.vertices)}, F={self.num_faces}, device={self.device})"

    def _rays(self, rays, mode: int):
        """the checks every query makes -> (rays [N,6] float32 contiguous on the mesh's device, the leading shape, whether the caller passed numpy)"""
        if mode not in (0, 1):
            raise RuntimeError(f"mode is 0 (the tree) or 1 (every face), got {mode!r}")
        as_numpy = not isinstance(rays, torch.Tensor)
        if as_numpy:
            rays = np.asarray(rays)
            if rays.ndim < 1 or rays.shape[-1] != 6 or rays.dtype.kind != "f":
                raise RuntimeError(f"expected floating rays of shape [...,6] (origin, direction), got {rays.dtype} {rays.shape}")
        elif rays.dtype != torch.float32 or rays.dim() < 1 or rays.shape[-1] != 6:
            raise RuntimeError(f"expected float32 rays of shape [...,6] (origin, direction), got {rays.dtype} {tuple(rays.shape)}")
        if self._sdf is None:
            raise RuntimeError("the scene has no mesh: call add_triangles(vertices, faces) first")
        dev = self._sdf.device
        if dev is None:
            raise RuntimeError("youreditableavatar_amd.mesh_rays answers queries on a HIP device only, and none is available: the tree was built, nothing can walk it")
        lead = tuple(rays.shape[:-1])
        if as_numpy:
            rays = torch.from_numpy(np.array(rays, dtype=np.float32, order="C")).to(dev)            # (a copy: the caller's array may be read-only)
        elif _need_device("mesh_rays", rays=rays) != dev:                         # a CPU tensor raises there: a host caller passes numpy
            raise RuntimeError(f"the mesh is on {dev}, rays on {rays.device}")
        return rays.detach().reshape(-1, 6).contiguous(), lead, as_numpy

    def _cast(self, rays: torch.Tensor, mode: int, t=None, face=None, geom=None, uv=None, normal=None, hit=None) -> None:
        N = int(rays.shape[0])
        if N == 0:
            return
        dev = self._sdf.device
        v, f, tree = self._sdf._dev
        with _guard(dev):
            _ok(_lib.tgs_meshrays_cast(_raw_stream(dev.index), tree.data_ptr(), self._sdf._bytes, v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), 0, N, rays.data_ptr(), mode,
                                       *(_host.ptr(x) for x in (t, face, geom, uv, normal, hit))))

    def cast_rays(self, rays, mode: int = 0) -> dict:
        """``rays`` [...,6] -> dict(``t_hit`` float32 [...], ``geometry_ids`` [...], ``primitive_ids`` [...], ``primitive_uvs`` float32 [...,2],
        ``primitive_normals`` float32 [...,3]).  A float32 tensor on the mesh's device gives tensors on that device, enqueued on the current stream with no host
        read-back, the ids int32 with -1 for a miss.  A numpy array gives numpy arrays, the ids viewed as uint32, so that ``ids < INVALID_ID`` works as the
        reference writes it.  A miss: ``t_hit`` +inf, uvs and normals 0.  ``mode=1`` visits every face (the cross-check): same bits."""
        r, lead, as_numpy = self._rays(rays, mode)
        dev, N = r.device, int(r.shape[0])
        out = dict(t_hit=torch.empty(N, dtype=torch.float32, device=dev), geometry_ids=torch.empty(N, dtype=torch.int32, device=dev),
                   primitive_ids=torch.empty(N, dtype=torch.int32, device=dev), primitive_uvs=torch.empty((N, 2), dtype=torch.float32, device=dev),
                   primitive_normals=torch.empty((N, 3), dtype=torch.float32, device=dev))
        self._cast(r, mode, out["t_hit"], out["primitive_ids"], out["geometry_ids"], out["primitive_uvs"], out["primitive_normals"])
        out = {k: out[k].reshape(lead + tuple(out[k].shape[1:])) for k in _KEYS}
        if as_numpy:
            out = {k: a.cpu().numpy() for k, a in out.items()}
            out["geometry_ids"], out["primitive_ids"] = out["geometry_ids"].view(np.uint32), out["primitive_ids"].view(np.uint32)
        return out

    def test_occlusions(self, rays, tnear: float = 0.0, tfar: float = float("inf"), mode: int = 0):
        """-> bool [...]: some face has a hit with ``tnear <= t <= tfar`` (both read as float32)"""
        r, lead, as_numpy = self._rays(rays, mode)
        tnear, tfar = float(np.float32(tnear)), float(np.float32(tfar))
        if not tnear <= tfar:
            raise RuntimeError(f"tnear <= tfar required, neither a NaN; got {tnear!r}, {tfar!r}")
        dev, N = r.device, int(r.shape[0])
        out = torch.empty(N, dtype=torch.bool, device=dev)
        if N:
            v, f, tree = self._sdf._dev
            with _guard(dev):
                _ok(_lib.tgs_meshrays_occluded(_raw_stream(dev.index), tree.data_ptr(), self._sdf._bytes, v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), 0, N, r.data_ptr(),
                                               tnear, tfar, mode, out.data_ptr()))
        out = out.reshape(lead)
        return out.cpu().numpy() if as_numpy else out

    def hit_faces(self, rays, out=None, mode: int = 0) -> torch.Tensor:
        """-> bool [F] on the mesh's device: the faces some ray hits first, the reference's ``hit_tri_id_all_set`` as ``mesh_region.refine_region`` takes it.
        ``out``: a previous camera's array, which is ORed into and returned.  One launch, nothing else is written, nothing is read back."""
        r, _, _ = self._rays(rays, mode)
        F = self.num_faces
        if out is None:
            out = torch.zeros(F, dtype=torch.bool, device=r.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.bool or tuple(out.shape) != (F,) or not out.is_contiguous() or out.device != r.device:
            got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
            raise RuntimeError(f"expected out as a contiguous bool tensor of shape [F] = [{F}] on {r.device}, got {got}")
        self._cast(r, mode, hit=out)
        return out

    def count_intersections(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("count_intersections"))

    def list_intersections(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("list_intersections"))

    def compute_closest_points(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("compute_closest_points"))

    def compute_distance(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("compute_distance"))

    def compute_signed_distance(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("compute_signed_distance"))

    def compute_occupancy(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("compute_occupancy"))
