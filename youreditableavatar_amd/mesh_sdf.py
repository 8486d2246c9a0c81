"""Signed distance from points to a triangle mesh: the target of the geometry stage's shape initialisation, with the call shape of ``pysdf.SDF``.

``ImplicitSDF.initialize_shape`` (``tetgs_spatial/models/geometry/implicit_sdf.py`` :231-239) fits the field to ``pysdf.SDF(mesh.vertices, mesh.faces)``
15 501 times, each time through ``points_rand.cpu().numpy()`` and ``torch.from_numpy(...).to(points_rand)``.  ``SDF`` here answers a numpy array with a
numpy array, so that line works with one changed import, and answers a device tensor with a device tensor on the current stream with no host read-back.
The kernels are ``csrc/tgs_mesh_sdf.hip``; the rules are written down in include/tgs_raster.h, "mesh signed distance", and restated in
tests/mesh_sdf_ref.py.  The tree is built on the host, once per mesh; the queries run on a HIP device only: there is no CPU path.

What differs from pysdf (which nobody could run next to this; by its documentation): pysdf takes the distance from the faces around the nearest vertex,
which is approximate, and containment from ray casting; here the distance is the exact minimum over all faces, and a point is inside when at least two of
the three ray parities along +x, +y, +z are odd, which serves meshes with small holes; where two solids overlap, the overlap is outside.  Positive inside,
as pysdf has it.  ``robust=False``, ``nn``, ``sample_surface`` and ``surface_area`` are not served and raise.  No autograd: the target is a constant, and
``closest`` gives ``(p - c) / d`` to anyone who needs the derivative.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _host
from ._host import _I, _L, _P, _Z, guard as _guard, need_device as _need_device, ok as _ok, raw_stream as _raw_stream

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h and tgs_mesh_sdf_testing.h declare them (every pointer is a c_void_p)
    "tgs_meshsdf_tree_bytes": (_Z, [_I]),
    "tgs_meshsdf_max_faces": (_I, []),
    "tgs_meshsdf_build": (_I, [_I, _I, _P, _P, _I, _P, _Z]),
    "tgs_meshsdf_query": (_I, [_P, _P, _Z, _I, _I, _P, _P, _I, _L, _P, _I, _P, _P, _P, _P]),
    "tgs_meshsdf_query_host": (_I, [_P, _Z, _I, _I, _P, _P, _I, _L, _P, _I, _P, _P, _P, _P]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_FACES = int(_lib.tgs_meshsdf_max_faces())
MAX_VERTICES = (1 << 31) - 1
_NOT_SERVED = "youreditableavatar_amd.mesh_sdf.SDF does not serve {}: it serves __call__, contains, closest, vertices and faces"


def _host_array(name: str, a, dtype, kind: str) -> np.ndarray:
    """a numpy array or a tensor on any device -> a contiguous host array [M,3] of ``dtype`` (for a device tensor: the one copy to the host)"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in kind:
        raise RuntimeError(f"expected {name} of shape [{name[0].upper()},3] and {'a floating' if 'f' in kind else 'an integer'} type, got {a.dtype} {a.shape}")
    if dtype == np.int32 and a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise RuntimeError(f"{name} holds a vertex index outside [0, {MAX_VERTICES}]")
    return np.ascontiguousarray(a.astype(dtype, copy=False))


class SDF:
    """``SDF(vertices, faces)``: ``vertices`` [V,3] floats, all finite, ``faces`` [F,3] integer indices in ``[0, V)``, ``1 <= F <= MAX_FACES``; numpy arrays or
    tensors on any device (read as float32 and int32).  Builds the tree on the host, once, and keeps ``vertices``, ``faces`` and the tree on the HIP device of
    the inputs (host inputs: the current device).  A mesh the library refuses (a non-finite vertex, an index out of range, no faces) raises.  Without a
    HIP device the object is built and every query raises."""

    def __init__(self, vertices, faces, robust: bool = True):
        if not robust:
            raise NotImplementedError(_NOT_SERVED.format("robust=False (only the ray rule is served)"))
        devs = {a.device for a in (vertices, faces) if isinstance(a, torch.Tensor) and a.is_cuda}
        if len(devs) > 1:
            raise RuntimeError(f"vertices and faces are on different devices: {sorted(map(str, devs))}")
        self._vertices = _host_array("vertices", vertices, np.float32, "f")
        self._faces = _host_array("faces", faces, np.int32, "iu")
        V, F = len(self._vertices), len(self._faces)
        if not 1 <= F <= MAX_FACES:
            raise RuntimeError(f"faces has {F} rows; at least 1 and at most 2^28 - 1 = {MAX_FACES} (code -1)")
        self._bytes = int(_lib.tgs_meshsdf_tree_bytes(F))
        self._tree = np.empty(self._bytes, dtype=np.uint8)
        _ok(_lib.tgs_meshsdf_build(V, F, self._vertices.ctypes.data, self._faces.ctypes.data, 0, self._tree.ctypes.data, self._bytes))
        self.device = next(iter(devs)) if devs else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        if self.device is not None:
            self._dev = tuple(torch.from_numpy(a).to(self.device) for a in (self._vertices, self._faces, self._tree))

    vertices = property(lambda self: self._vertices, doc="[V,3] float32, on the host, as the queries read them")
    faces = property(lambda self: self._faces, doc="[F,3] int32, on the host")

    def __repr__(self):
        return f"SDF(V={len(self._vertices)}, F={len(self._faces)}, device={self.device})"

    def _query(self, points, mode: int, want: str):
        """``want``: some of 's' (sdf), 'f' (face), 'c' (closest), 'i' (inside) -> those outputs in that order, as numpy arrays for a numpy ``points``"""
        if mode not in (0, 1):
            raise RuntimeError(f"mode is 0 (the tree) or 1 (every face), got {mode!r}")
        as_numpy = not isinstance(points, torch.Tensor)
        if as_numpy:
            points = np.asarray(points)
            if points.ndim != 2 or points.shape[1] != 3 or points.dtype.kind != "f":
                raise RuntimeError(f"expected floating points of shape [N,3], got {points.dtype} {points.shape}")
        elif points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            raise RuntimeError(f"expected float32 points of shape [N,3], got {points.dtype} {tuple(points.shape)}")
        if self.device is None:
            raise RuntimeError("youreditableavatar_amd.mesh_sdf answers queries on a HIP device only, and none is available: the tree was built, nothing can walk it")
        if as_numpy:
            points = torch.from_numpy(np.ascontiguousarray(points.astype(np.float32, copy=False))).to(self.device)
        elif _need_device("mesh_sdf", points=points) != self.device:           # a CPU tensor raises there: a host caller passes numpy
            raise RuntimeError(f"the mesh is on {self.device}, points on {points.device}")
        dev, N = self.device, int(points.shape[0])
        kinds = {"s": ((N,), torch.float32), "f": ((N,), torch.int32), "c": ((N, 3), torch.float32), "i": ((N,), torch.bool)}
        out = {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=dev) for k in want}
        if N:
            points = points.detach().contiguous()
            v, f, tree = self._dev
            with _guard(dev):
                _ok(_lib.tgs_meshsdf_query(_raw_stream(dev.index), tree.data_ptr(), self._bytes, v.shape[0], f.shape[0], v.data_ptr(), f.data_ptr(), 0, N, points.data_ptr(), mode,
                                           *(out[k].data_ptr() if k in out else None for k in "sfci")))
        res = tuple(out[k].cpu().numpy() if as_numpy else out[k] for k in want)
        return res[0] if len(res) == 1 else res

    def __call__(self, points, mode: int = 0):
        """``points`` [N,3] -> the signed distance [N] float32, positive inside.  A numpy array gives a numpy array; a float32 tensor on the mesh's device
        gives a tensor on that device, enqueued on the current stream with no host read-back.  ``mode=1`` visits every face (the cross-check): same bits."""
        return self._query(points, mode, "s")

    def contains(self, points, mode: int = 0):
        """-> bool [N]: at least two of the three ray parities are odd, or the point is on the mesh"""
        return self._query(points, mode, "i")

    def closest(self, points, mode: int = 0):
        """-> ``(sdf [N] float32, face [N] int32, closest [N,3] float32)``: the lowest face at the least distance and its closest point; a non-finite
        point gives NaN, -1, NaN"""
        return self._query(points, mode, "sfc")

    def nn(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("nn"))

    def sample_surface(self, *args, **kwargs):
        raise NotImplementedError(_NOT_SERVED.format("sample_surface"))

    @property
    def surface_area(self):
        raise NotImplementedError(_NOT_SERVED.format("surface_area"))
