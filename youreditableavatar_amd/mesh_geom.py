"""Mesh normals, edges and smoothness losses for the geometry stage, with gradients: the link between ``marching_tets`` and the mesh rasterizer.

``vertex_normals(v_pos, faces)`` is the body of ``compute_normal`` / ``compute_vertex_normal`` (``tetgs_spatial/models/renderers/nvdiff_rasterize_utils.py``
:12-35, :37-70), of ``Mesh._compute_vertex_normal`` (``models/mesh.py`` :136-162) and of the painting stage's ``compute_normal``; ``mesh_topology(...).edges``
is ``Mesh._compute_edges`` (:261-273); ``normal_consistency`` and ``laplacian`` are the two ``Mesh`` losses of the same names (:275-315).  The kernels are
``csrc/tgs_mesh_geom.hip``; the rules are written down in include/tgs_raster.h, "mesh geometry", and restated in tests/mesh_geom_ref.py.  HIP device only:
there is no CPU path.  float32 values; ``faces`` int32 or int64, read as given.

What differs from the reference's framework ops: a ``MeshTopology`` is built once per mesh (one read-back: the number of edges and the index flag) and
every call on that mesh reads nothing back; an index outside ``[0, V)`` raises instead of faulting; the cross product is always along the last axis
(``torch.cross`` without ``dim`` picks the first axis of size 3, so with exactly 3 faces the reference crosses along the wrong one); there are no float
atomics, so two runs give the same bits, forward and backward.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _host
from ._host import _I, _L, _P, _Z, guard as _guard, index_error as _index_error, need_device as _need_device, ok as _ok, raw_stream as _raw_stream

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_meshgeom_workspace_bytes": (_Z, [_I, _I]),
    "tgs_meshgeom_table_bytes": (_Z, [_I]),
    "tgs_meshgeom_normals_backward_workspace_bytes": (_Z, [_I, _I]),
    "tgs_meshgeom_topology_count": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _Z, _P, _Z]),
    "tgs_meshgeom_topology_fill": (_I, [_P, _I, _I, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _Z]),
    "tgs_meshgeom_normals": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "tgs_meshgeom_normals_backward": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _Z]),
    "tgs_meshgeom_consistency": (_I, [_P, _I, _L, _P, _P, _P, _P, _Z]),
    "tgs_meshgeom_consistency_backward": (_I, [_P, _I, _L, _P, _P, _P, _P, _P, _P, _P]),
    "tgs_meshgeom_laplacian": (_I, [_P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _Z]),
    "tgs_meshgeom_laplacian_backward": (_I, [_P, _I, _L, _P, _P, _P, _P, _P, _P, _P]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_VERTICES = (1 << 31) - 1
MAX_FACES = ((1 << 32) - 1) // 3   # incidence entries 3 * face + corner and edge numbers are 32-bit


def _check_faces(faces) -> int:
    if not isinstance(faces, torch.Tensor):
        raise RuntimeError("faces must be a tensor")
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"expected int32 or int64 faces of shape [F,3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.shape[0] > MAX_FACES:
        raise RuntimeError(f"faces has {faces.shape[0]} rows; at most (2^32 - 1) / 3 = {MAX_FACES}")
    return int(faces.shape[0])


def _check_rows(name: str, t) -> int:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"expected float32 {name} of shape [V,3], got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] > MAX_VERTICES:
        raise RuntimeError(f"{name} has {t.shape[0]} rows; at most 2^31 - 1")
    return int(t.shape[0])


class MeshTopology:
    """What ``mesh_topology`` built for one ``faces`` array: ``edges`` [E,2] int64 (``None`` when built with ``edges=False``), and, for the kernels, the
    vertex -> (face, corner) incidence (``inc_end`` [V+1], ``inc`` [3F]: the runs' ends and the entries ``3 * face + corner``) and the edges' runs
    (``edge_end``, ``max_end`` [V+1], ``max_list`` [E]), all 32-bit words held in int32 tensors.  ``num_vertices``, ``num_faces``, ``num_edges``, ``device``."""
    __slots__ = ("num_vertices", "num_faces", "num_edges", "device", "inc_end", "inc", "edges", "edge_end", "max_end", "max_list")

    def __init__(self, V, F, E, device, inc_end, inc, edges, edge_end, max_end, max_list):
        self.num_vertices, self.num_faces, self.num_edges, self.device = V, F, E, device
        self.inc_end, self.inc, self.edges, self.edge_end, self.max_end, self.max_list = inc_end, inc, edges, edge_end, max_end, max_list

    @property
    def has_edges(self) -> bool:
        return self.edges is not None

    def __repr__(self):
        return f"MeshTopology(V={self.num_vertices}, F={self.num_faces}, E={self.num_edges if self.has_edges else None}, device={self.device})"


def _workspace(V: int, F: int, dev: torch.device):
    return _host.workspace(_lib.tgs_meshgeom_workspace_bytes(V, F), dev)


def _faces_arg(faces: torch.Tensor):
    faces = faces.contiguous()
    return faces, int(faces.dtype == torch.int64)


def mesh_topology(faces: torch.Tensor, num_vertices: int, edges: bool = True) -> MeshTopology:
    """``faces`` [F,3] int32 or int64 on a HIP device, the mesh's number of vertices -> the ``MeshTopology`` every call below takes.  One read-back
    (the number of edges and the index flag); an index outside ``[0, num_vertices)`` raises a ``RuntimeError`` after it.  ``edges=False``: the incidence
    alone, which is all ``vertex_normals`` reads.  ``F = 0`` or ``V = 0``: an empty topology, no native call."""
    F = _check_faces(faces)
    if isinstance(num_vertices, bool) or not isinstance(num_vertices, int) or not 0 <= num_vertices <= MAX_VERTICES:
        raise RuntimeError(f"num_vertices must be an int in [0, 2^31 - 1], got {num_vertices!r}")
    V = num_vertices
    dev = _need_device("mesh_geom", faces=faces)
    words = lambda n, zero=False: (torch.zeros if zero else torch.empty)((n,), dtype=torch.int32, device=dev)
    if F and not V:
        raise _index_error("faces", V, f"the mesh has {V} vertices")
    if not F:
        return MeshTopology(V, F, 0, dev, words(V + 1, True), words(0), torch.empty((0, 2), dtype=torch.int64, device=dev) if edges else None,
                            words(V + 1, True), words(V + 1, True), words(0))
    faces, is64 = _faces_arg(faces)
    with _guard(dev):
        st = _raw_stream(dev.index)
        ws, nbytes = _workspace(V, F, dev)
        counts = torch.empty((4,), dtype=torch.int64, device=dev)
        inc_end, edge_end, max_end = words(V + 1), words(V + 1 if edges else 0), words(V + 1 if edges else 0)
        table, tbytes = None, 0
        if edges:
            table, tbytes = _host.workspace(_lib.tgs_meshgeom_table_bytes(F), dev)
        _ok(_lib.tgs_meshgeom_topology_count(st, V, F, faces.data_ptr(), is64, inc_end.data_ptr(), edge_end.data_ptr() if edges else None,
                                              max_end.data_ptr() if edges else None, counts.data_ptr(), table.data_ptr() if edges else None, tbytes, ws.data_ptr(), nbytes))
        E, bad, _, _ = counts.tolist()                                          # the read-back
        if bad:
            raise _index_error("faces", V, f"the mesh has {V} vertices")
        inc, edge_rows, max_list = words(3 * F), torch.empty((E, 2), dtype=torch.int64, device=dev) if edges else None, words(E)
        _ok(_lib.tgs_meshgeom_topology_fill(st, V, F, faces.data_ptr(), is64, E, inc_end.data_ptr(), inc.data_ptr(), edge_end.data_ptr() if edges else None,
                                             max_end.data_ptr() if edges else None, edge_rows.data_ptr() if edges else None, max_list.data_ptr() if edges else None,
                                             table.data_ptr() if edges else None, tbytes))
    return MeshTopology(V, F, E, dev, inc_end, inc, edge_rows, edge_end, max_end, max_list)


def _is_topology(topology) -> None:
    if not isinstance(topology, MeshTopology):
        raise RuntimeError(f"topology must be a MeshTopology (mesh_topology(faces, num_vertices)), got {type(topology).__name__}")


def _check_topology(topology, V: int, F: Optional[int], dev: torch.device, need_edges: bool) -> None:
    _is_topology(topology)
    if topology.num_vertices != V or (F is not None and topology.num_faces != F):
        raise RuntimeError(f"the topology was built for {topology.num_vertices} vertices and {topology.num_faces} faces, the call has {V}" + (f" and {F}" if F is not None else ""))
    if need_edges and not topology.has_edges:
        raise RuntimeError("the topology was built with edges=False: this call needs the edges")
    if topology.device != dev:
        raise RuntimeError(f"the topology is on {topology.device}, the values on {dev}")


# ---- vertex normals --------------------------------------------------------------------------------------------------------------------
def _check_normals(v_pos, faces, topology):
    V, F = _check_rows("v_pos", v_pos), _check_faces(faces)
    if topology is not None:
        _is_topology(topology)
    dev = _need_device("mesh_geom", v_pos=v_pos, faces=faces)
    if topology is None:
        topology = mesh_topology(faces, V, edges=False)
    _check_topology(topology, V, F, dev, False)
    return V, F, dev, topology


def _normals_forward(v_pos, faces, topo, V, F, dev):
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if not V:
        return out
    if not F:
        out[:] = torch.tensor([0.0, 0.0, 1.0], device=dev)
        return out
    v_pos = v_pos.contiguous()
    faces, is64 = _faces_arg(faces)
    with _guard(dev):
        _ok(_lib.tgs_meshgeom_normals(_raw_stream(dev.index), V, F, v_pos.data_ptr(), faces.data_ptr(), is64, topo.inc_end.data_ptr(), topo.inc.data_ptr(), out.data_ptr()))
    return out


class _VertexNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, faces, topo, V, F, dev):
        ctx.args = (faces, topo, V, F, dev)
        ctx.save_for_backward(v_pos)
        return _normals_forward(v_pos.detach(), faces, topo, V, F, dev)

    @staticmethod
    def backward(ctx, g):
        (v_pos,) = ctx.saved_tensors
        faces, topo, V, F, dev = ctx.args
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        if not V or not F:
            return (torch.zeros((V, 3), dtype=torch.float32, device=dev),) + (None,) * 5
        d_pos = torch.empty((V, 3), dtype=torch.float32, device=dev)
        p, g = v_pos.detach().contiguous(), g.contiguous()
        faces, is64 = _faces_arg(faces)
        with _guard(dev):
            ws, nbytes = _host.workspace(_lib.tgs_meshgeom_normals_backward_workspace_bytes(V, F), dev)
            _ok(_lib.tgs_meshgeom_normals_backward(_raw_stream(dev.index), V, F, p.data_ptr(), faces.data_ptr(), is64, topo.inc_end.data_ptr(), topo.inc.data_ptr(),
                                                    g.data_ptr(), d_pos.data_ptr(), ws.data_ptr(), nbytes))
        return (d_pos,) + (None,) * 5


def vertex_normals(v_pos: torch.Tensor, faces: torch.Tensor, topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``v_pos`` [V,3] float32, ``faces`` [F,3] int32 or int64, on one HIP device -> the vertex normals [V,3] float32, differentiable with respect to
    ``v_pos``: the normalized sum of the incident face normals, ``(0, 0, 1)`` where the sum's squared length is not ``> 1e-20``.  ``topology=None``
    builds the incidence here (one read-back).  Under ``no_grad``, or with ``v_pos`` requiring no gradient, it is the forward alone."""
    V, F, dev, topo = _check_normals(v_pos, faces, topology)
    if torch.is_grad_enabled() and v_pos.requires_grad:
        return _VertexNormals.apply(v_pos, faces, topo, V, F, dev)
    return _normals_forward(v_pos.detach(), faces, topo, V, F, dev)


# ---- normal consistency ----------------------------------------------------------------------------------------------------------------
def _consistency_forward(v_nrm, topo, V, dev):
    E = topo.num_edges
    if not E:                                                                   # the mean of nothing, as the reference gives it
        return torch.full((), float("nan"), dtype=torch.float32, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    v_nrm = v_nrm.contiguous()
    with _guard(dev):
        ws, nbytes = _workspace(V, topo.num_faces, dev)
        _ok(_lib.tgs_meshgeom_consistency(_raw_stream(dev.index), V, E, v_nrm.data_ptr(), topo.edges.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes))
    return out


class _Consistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_nrm, topo, V, dev):
        ctx.args = (topo, V, dev)
        ctx.save_for_backward(v_nrm)
        return _consistency_forward(v_nrm.detach(), topo, V, dev)

    @staticmethod
    def backward(ctx, g):
        (v_nrm,) = ctx.saved_tensors
        topo, V, dev = ctx.args
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if not topo.num_edges:
            return torch.zeros((V, 3), dtype=torch.float32, device=dev), None, None, None
        d_nrm = torch.empty((V, 3), dtype=torch.float32, device=dev)
        n, g = v_nrm.detach().contiguous(), g.to(torch.float32).contiguous()
        with _guard(dev):
            _ok(_lib.tgs_meshgeom_consistency_backward(_raw_stream(dev.index), V, topo.num_edges, n.data_ptr(), topo.edges.data_ptr(), topo.edge_end.data_ptr(),
                                                        topo.max_end.data_ptr(), topo.max_list.data_ptr(), g.data_ptr(), d_nrm.data_ptr()))
        return d_nrm, None, None, None


def normal_consistency(v_nrm: torch.Tensor, topology: MeshTopology) -> torch.Tensor:
    """``v_nrm`` [V,3] float32 and the mesh's topology (with edges) -> the 0-dim mean over ``topology.edges`` of ``1 - cosine_similarity(n_a, n_b)``,
    differentiable with respect to ``v_nrm``.  No edges: NaN, the mean of nothing."""
    V = _check_rows("v_nrm", v_nrm)
    _is_topology(topology)
    dev = _need_device("mesh_geom", v_nrm=v_nrm)
    _check_topology(topology, V, None, dev, True)
    if torch.is_grad_enabled() and v_nrm.requires_grad:
        return _Consistency.apply(v_nrm, topology, V, dev)
    return _consistency_forward(v_nrm.detach(), topology, V, dev)


def mesh_normal_consistency(v_pos: torch.Tensor, faces: torch.Tensor, topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``Mesh(v_pos, faces).normal_consistency()``: ``normal_consistency(vertex_normals(v_pos, faces, topology), topology)``"""
    if topology is None:
        _check_rows("v_pos", v_pos), _check_faces(faces)
        _need_device("mesh_geom", v_pos=v_pos, faces=faces)
        topology = mesh_topology(faces, int(v_pos.shape[0]))
    return normal_consistency(vertex_normals(v_pos, faces, topology), topology)


# ---- the uniform Laplacian -------------------------------------------------------------------------------------------------------------
def _laplacian_forward(v_pos, topo, V, dev, keep: bool):
    """-> (the loss, the unit rows [V,3] float64 the backward gathers over or None)"""
    if not V:
        return torch.full((), float("nan"), dtype=torch.float32, device=dev), None
    if not topo.num_edges:                                                      # every row is zero: no native call
        return torch.zeros((), dtype=torch.float32, device=dev), None
    out = torch.empty((), dtype=torch.float32, device=dev)
    unit = torch.empty((V, 3), dtype=torch.float64, device=dev) if keep else None
    v_pos = v_pos.contiguous()
    with _guard(dev):
        ws, nbytes = _workspace(V, topo.num_faces, dev)
        _ok(_lib.tgs_meshgeom_laplacian(_raw_stream(dev.index), V, topo.num_edges, v_pos.data_ptr(), topo.edges.data_ptr(), topo.edge_end.data_ptr(),
                                         topo.max_end.data_ptr(), topo.max_list.data_ptr(),
                                         unit.data_ptr() if keep else None, out.data_ptr(), ws.data_ptr(), nbytes))
    return out, unit


class _Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, topo, V, dev):
        out, unit = _laplacian_forward(v_pos.detach(), topo, V, dev, True)
        ctx.args = (topo, V, dev, unit)
        return out

    @staticmethod
    def backward(ctx, g):
        topo, V, dev, unit = ctx.args
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if unit is None:                                                        # no vertices or no edges: the zero subgradient
            return torch.zeros((V, 3), dtype=torch.float32, device=dev), None, None, None
        d_pos = torch.empty((V, 3), dtype=torch.float32, device=dev)
        g = g.to(torch.float32).contiguous()
        with _guard(dev):
            _ok(_lib.tgs_meshgeom_laplacian_backward(_raw_stream(dev.index), V, topo.num_edges, topo.edges.data_ptr(), topo.edge_end.data_ptr(), topo.max_end.data_ptr(),
                                                      topo.max_list.data_ptr(), unit.data_ptr(), g.data_ptr(), d_pos.data_ptr()))
        return d_pos, None, None, None


def laplacian(v_pos: torch.Tensor, topology: MeshTopology) -> torch.Tensor:
    """``v_pos`` [V,3] float32 and the mesh's topology (with edges) -> ``Mesh.laplacian()``: the 0-dim mean over the vertices of the norm of the uniform
    Laplacian's row, ``sum over the distinct neighbours o != v of (v_pos[v] - v_pos[o])``, differentiable with respect to ``v_pos``; a zero row gets the
    zero subgradient.  No vertices: NaN, the mean of nothing."""
    V = _check_rows("v_pos", v_pos)
    _is_topology(topology)
    dev = _need_device("mesh_geom", v_pos=v_pos)
    _check_topology(topology, V, None, dev, True)
    if torch.is_grad_enabled() and v_pos.requires_grad:
        return _Laplacian.apply(v_pos, topology, V, dev)
    return _laplacian_forward(v_pos.detach(), topology, V, dev, False)[0]
