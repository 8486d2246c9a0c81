"""Tetrahedral grids for the geometry stage: the compaction around the surface, the 8x subdivision and the keep / edit split.

``compact_tets`` and ``batch_subdivide_volume`` return what the methods of that name of ``MarchingTetrahedraHelper`` return
(``tetgs_spatial/models/isosurface.py`` :264-345), so each method's body becomes one ``return``; ``mark_part_tets`` returns the dict of the method
of that name (:208-261).  ``subdivide_tets`` is the unbatched call under ``batch_subdivide_volume``.  The kernels are ``csrc/tgs_tet_grid.hip``;
the rules are written down in include/tgs_raster.h, "tetrahedral grids", and restated in tests/tet_ref.py.  HIP device only: no CPU path.

What differs from the reference's framework ops: each call reads a handful of integers back once (the output sizes with the index flag), where
every data-dependent size of the reference -- a boolean-mask index, a ``torch.unique`` -- is a read-back of its own; an index outside ``[0, N)``
raises instead of faulting; ``compact_tets`` has the keywords ``threshold`` (the reference's constant 0.02) and ``index_dtype``;
``subdivide_tets`` also returns ``edges``; ``mark_part_tets`` takes membership by vertex index, not by coordinates.  Everything is integer
topology, bit copies and exact halvings, so the outputs equal the reference's element for element and two runs give the same bits.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _host
from ._host import _F, _I, _L, _P, _Z, guard as _guard, index_error as _index_error, index_rows as _rows, ok as _ok, ptr as _ptr, raw_stream as _raw_stream, workspace as _workspace
from .marching_tets import MASK_TYPES, MAX_ROWS, check, marching_tets

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_tet_compact_workspace_bytes": (_Z, [_I, _I]),
    "tgs_tet_compact_select": (_I, [_P, _I, _I, _P, _P, _I, _P, _F, _P, _P, _Z]),
    "tgs_tet_compact_emit": (_I, [_P, _I, _I, _P, _I, _L, _L, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z]),
    "tgs_tet_subdivide_workspace_bytes": (_Z, [_I, _I]),
    "tgs_tet_subdivide_edges": (_I, [_P, _I, _I, _P, _I, _P, _P, _Z]),
    "tgs_tet_subdivide_emit": (_I, [_P, _I, _I, _I, _L, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _Z]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_SUBDIV_TETS = MAX_ROWS // 8                                                 # new_tets has 8 F rows
MARK_KEYS = ("keep_verts_indices", "keep_pos", "keep_sdf", "keep_tets", "keep_tet_idx", "unique_grid_vtx", "new_pos", "new_sdf", "new_tets", "mask_keep_part_in_new_pos")


def _check(named, N: Optional[int] = None) -> torch.device:
    """``named``: (name, tensor, kind) with kind in pos / sdf / tet / mask -> the one device of all of them (``marching_tets.check`` has the rules)"""
    return check("tet_grid", named, N)


class _Selection:
    """one select call: the counts read back, and the workspace that the emit (or another selection's membership) reads"""

    def __init__(self, dev, N, F, tet, sdf=None, keep=None, threshold=0.0):
        self.dev, self.N, self.F, self.tet = dev, N, F, tet
        self.n_tets = self.n_verts = 0
        self.ws, self.nbytes = _workspace(_lib.tgs_tet_compact_workspace_bytes(N, F), dev)
        if F == 0:
            return
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        with _guard(dev):
            _ok(_lib.tgs_tet_compact_select(_raw_stream(dev.index), N, F, _ptr(sdf), tet.data_ptr(), int(tet.dtype == torch.int64), _ptr(keep), float(threshold),
                                            counts.data_ptr(), self.ws.data_ptr(), self.nbytes))
        self.n_tets, self.n_verts, bad, _ = counts.tolist()                      # the read-back
        if bad:
            raise _index_error("tet", N, f"pos has {N} rows")

    def emit(self, index_dtype, pos=None, sdf=None, mask=None, member_of: Optional["_Selection"] = None):
        """-> (new_tets, new_tet_idx_to_old, unique_vtx, new_pos, new_sdf [N'], new_mask [N'], member [N'] int32), None for what was not given"""
        dev, Fk, Nk = self.dev, self.n_tets, self.n_verts
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = [new((Fk, 4), index_dtype), new((Fk,), index_dtype), new((Nk,), index_dtype), None if pos is None else new((Nk, 3), torch.float32),
               None if sdf is None else new((Nk,), torch.float32), None if mask is None else new((Nk,), mask.dtype), None if member_of is None else new((Nk,), torch.int32)]
        if Fk == 0:
            return out
        with _guard(dev):
            _ok(_lib.tgs_tet_compact_emit(_raw_stream(dev.index), self.N, self.F, self.tet.data_ptr(), int(self.tet.dtype == torch.int64), Fk, Nk, _ptr(pos), _ptr(sdf),
                                          _ptr(mask), MASK_TYPES[mask.dtype] if mask is not None else 0, None if member_of is None else member_of.ws.data_ptr(),
                                          int(index_dtype == torch.int64), *(_ptr(t) for t in out), self.ws.data_ptr(), self.nbytes))
        return out


def _index_dtype(index_dtype) -> torch.dtype:
    if index_dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"index_dtype must be torch.int32 or torch.int64, got {index_dtype}")
    return index_dtype


@torch.no_grad()
def compact_tets(pos: torch.Tensor, sdf: torch.Tensor, tet: torch.Tensor, mask: Optional[torch.Tensor] = None, threshold: float = 0.02,
                 index_dtype: torch.dtype = torch.int64):
    """``pos`` [N,3] float32, ``sdf`` [N] or [N,1] float32, ``tet`` [F,4] int32 or int64, ``mask`` [N] or [N,1] (int32, int64, float32 or one byte)
    or None, on one HIP device -> ``(new_pos, new_sdf, new_tets, new_mask, new_tet_idx_to_old)``: the tetrahedra whose |mean sdf| is at most
    ``threshold`` (compared in float32; a NaN mean is dropped), renumbered over their own vertices, which keep their ascending order; ``new_sdf``
    and ``new_mask`` keep the shapes of ``sdf`` and ``mask``; the index outputs are ``index_dtype``.  One read-back.  The outputs are detached
    whatever the inputs require, as the reference's method runs under ``no_grad``.  Nothing kept: [0,3], [0] or [0,1], [0,4], [0]."""
    named = [("pos", pos, "pos"), ("sdf", sdf, "sdf"), ("tet", tet, "tet")] + ([("mask", mask, "mask")] if mask is not None else [])
    dev = _check(named, int(pos.shape[0]) if isinstance(pos, torch.Tensor) else None)
    index_dtype = _index_dtype(index_dtype)
    N, F = int(pos.shape[0]), int(tet.shape[0])
    p, s, t = pos.detach().contiguous(), sdf.detach().reshape(-1).contiguous(), _rows(tet)
    m = None if mask is None else mask.detach().reshape(-1).contiguous()
    sel = _Selection(dev, N, F, t, sdf=s, threshold=threshold)
    new_tets, to_old, _, new_pos, new_sdf, new_mask, _ = sel.emit(index_dtype, p, s, m)
    shaped = lambda out, like: out.reshape(-1, 1) if like.dim() == 2 else out
    return new_pos, shaped(new_sdf, sdf), new_tets, None if mask is None else shaped(new_mask, mask), to_old


def _subdivide(pos: torch.Tensor, tet: torch.Tensor, mask: Optional[torch.Tensor]):
    """pos [B,N,3], tet [F,4], mask [B,N] or None, checked -> (new_v [B,N+E,3], new_tets [8F,4], new_mask [B,N+E] or None, sub_to_parent, edges)"""
    dev, B, N, F = pos.device, int(pos.shape[0]), int(pos.shape[1]), int(tet.shape[0])
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    if F > MAX_SUBDIV_TETS:
        raise RuntimeError(f"tet has {F} rows and the subdivision 8 times as many; at most 2^31 - 1")
    if F == 0:
        return pos, new((0, 4), torch.int64), None if mask is None else mask.float(), new((0,), torch.int64), new((0, 2), torch.int64)
    p, t = pos.detach().contiguous(), _rows(tet)
    m = None if mask is None else mask.detach().contiguous()
    with _guard(dev):
        st = _raw_stream(dev.index)
        ws, nbytes = _workspace(_lib.tgs_tet_subdivide_workspace_bytes(N, F), dev)
        counts = new((4,), torch.int64)
        is64 = int(t.dtype == torch.int64)
        _ok(_lib.tgs_tet_subdivide_edges(st, N, F, t.data_ptr(), is64, counts.data_ptr(), ws.data_ptr(), nbytes))
        E, bad, _, _ = counts.tolist()                                           # the read-back
        if bad:
            raise _index_error("tet", N, f"pos has {N} rows")
        if N + E > MAX_ROWS:
            raise RuntimeError(f"{N} vertices and {E} edges: new_v would have more than 2^31 - 1 rows")
        new_v, new_tets, sub, edges = new((B, N + E, 3), torch.float32), new((8 * F, 4), torch.int64), new((8 * F,), torch.int64), new((E, 2), torch.int64)
        new_mask = None if m is None else new((B, N + E), torch.float32)
        _ok(_lib.tgs_tet_subdivide_emit(st, N, F, B, E, p.data_ptr(), t.data_ptr(), is64, _ptr(m), MASK_TYPES[m.dtype] if m is not None else 0, new_v.data_ptr(),
                                        new_tets.data_ptr(), _ptr(new_mask), sub.data_ptr(), edges.data_ptr(), ws.data_ptr(), nbytes))
    return new_v, new_tets, new_mask, sub, edges


def subdivide_tets(pos: torch.Tensor, tet: torch.Tensor, mask: Optional[torch.Tensor] = None):
    """``pos`` [N,3] float32, ``tet`` [F,4] int32 or int64, ``mask`` [N] or [N,1] or None, on one HIP device ->
    ``(new_v [N+E,3], new_tets [8F,4] int64, new_mask [N+E,1] float32 or None, sub_to_parent [8F] int64, edges [E,2] int64)``: every
    tetrahedron cut into eight over the midpoints of its edges, ``new_v = [pos ; (pos[e0] + pos[e1]) * 0.5f]`` over the distinct edges in
    ascending (min, max) order, sub-tetrahedron k of parent f in row k F + f.  One read-back.  Where ``pos`` requires a gradient (and gradients
    are enabled) ``new_v`` is ``torch.cat([pos, pos[edges].mean(1)])`` over the native ``edges``: that is the framework's arithmetic and its
    autograd, there is no backward kernel; everything else stays native.  ``F = 0`` returns ``pos`` unchanged and [0,4]."""
    named = [("pos", pos, "pos"), ("tet", tet, "tet")] + ([("mask", mask, "mask")] if mask is not None else [])
    _check(named, int(pos.shape[0]) if isinstance(pos, torch.Tensor) else None)
    new_v, new_tets, new_mask, sub, edges = _subdivide(pos[None], tet, None if mask is None else mask.reshape(1, -1))
    new_v = new_v[0] if len(tet) else pos
    if torch.is_grad_enabled() and pos.requires_grad and len(edges):
        new_v = torch.cat([pos, pos[edges].mean(1)])
    return new_v, new_tets, None if new_mask is None else new_mask.reshape(-1, 1), sub, edges


def batch_subdivide_volume(tet_pos_bxnx3: torch.Tensor, tet_bxfx4: torch.Tensor, mask_keep_part_in_new_pos: Optional[torch.Tensor] = None):
    """``tet_pos_bxnx3`` [B,N,3], ``tet_bxfx4`` [B,F,4], mask [B,N,1] or None -> ``(new_v [B,N+E,3], tet [B,8F,4], new_mask [B,N+E,1] or None,
    sub_to_parent [8F])``, the reference's call shape.  Like the reference it takes the topology from ``tet_bxfx4[0]`` for every batch element:
    the topology runs once, the midpoints per element.  With positions that require a gradient the midpoints are the framework's (see
    ``subdivide_tets``)."""
    pos, tet, mask = tet_pos_bxnx3, tet_bxfx4, mask_keep_part_in_new_pos
    for name, t in (("tet_pos_bxnx3", pos), ("tet_bxfx4", tet)) + ((("mask_keep_part_in_new_pos", mask),) if mask is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] < 1:
            raise RuntimeError(f"expected {name} of shape [B,...,...] with B >= 1, got {f'{t.dtype} {tuple(t.shape)}' if isinstance(t, torch.Tensor) else type(t).__name__}")
    B, N = int(pos.shape[0]), int(pos.shape[1])
    if mask is not None and tuple(mask.shape) != (B, N, 1):
        raise RuntimeError(f"expected mask_keep_part_in_new_pos of shape [{B},{N},1], got {tuple(mask.shape)}")
    named = [("tet_pos_bxnx3", pos[0], "pos"), ("tet_bxfx4", tet[0], "tet")] + ([("mask_keep_part_in_new_pos", mask[0], "mask")] if mask is not None else [])
    _check(named, N)
    new_v, new_tets, new_mask, sub, edges = _subdivide(pos, tet[0], None if mask is None else mask.reshape(B, N))
    if torch.is_grad_enabled() and pos.requires_grad and len(edges):
        new_v = torch.cat([pos, pos[:, edges].mean(2)], 1)
    return new_v, new_tets[None].expand(B, -1, -1), None if new_mask is None else new_mask[..., None], sub


@torch.no_grad()
def mark_part_tets(grid_vertices: torch.Tensor, level: torch.Tensor, indices: torch.Tensor, edit_mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``grid_vertices`` [N,3] (the reference's grid with its deformation applied), ``level`` [N,1], ``indices`` [F,4], ``edit_mask`` [T] over the
    faces of ``marching_tets(grid_vertices, level, indices)`` -> the dict of the reference's method: the tetrahedra under a face with
    ``edit_mask == 0`` renumbered over their own vertices (``keep_*``), every other tetrahedron likewise (``unique_grid_vtx``, ``new_*``), and
    ``mask_keep_part_in_new_pos`` [N',1] int32, 1 where a vertex of the second part is also one of the first.  That membership is taken by
    vertex index, from the two selections' bitmaps, where the reference compares coordinate tuples in a Python set: the two agree whenever no
    two grid vertices share a position, which holds for any tetrahedral grid."""
    named = [("grid_vertices", grid_vertices, "pos"), ("level", level, "sdf"), ("indices", indices, "tet")]
    dev = _check(named, int(grid_vertices.shape[0]) if isinstance(grid_vertices, torch.Tensor) else None)
    pos, sdf, tet = grid_vertices.detach().contiguous(), level.detach().reshape(-1).contiguous(), _rows(indices)
    N, F = int(pos.shape[0]), int(tet.shape[0])
    f2t = marching_tets(pos, sdf, tet)["face_to_tet_idx"]
    if not isinstance(edit_mask, torch.Tensor) or edit_mask.device != dev or edit_mask.numel() != f2t.numel():
        raise RuntimeError(f"expected edit_mask on {dev} with one entry per face ({f2t.numel()}), got {tuple(edit_mask.shape) if isinstance(edit_mask, torch.Tensor) else type(edit_mask).__name__}")
    faces_kept = torch.zeros(F, dtype=torch.int32, device=dev).index_put_((f2t,), (edit_mask.reshape(-1) == 0).int(), accumulate=True)
    keep = (faces_kept > 0).to(torch.uint8)                                      # a tetrahedron with a kept face is kept
    first = _Selection(dev, N, F, tet, keep=keep)
    second = _Selection(dev, N, F, tet, keep=1 - keep)
    k_tets, k_idx, k_vtx, k_pos, k_sdf, _, _ = first.emit(torch.int64, pos, sdf)
    n_tets, _, n_vtx, n_pos, n_sdf, _, member = second.emit(torch.int64, pos, sdf, member_of=first)
    return dict(zip(MARK_KEYS, (k_vtx, k_pos, k_sdf.reshape(-1, 1), k_tets, k_idx, n_vtx, n_pos, n_sdf.reshape(-1, 1), n_tets, member.reshape(-1, 1))))
