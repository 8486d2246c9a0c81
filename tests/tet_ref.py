"""The tetrahedral grid's passes, restated in torch from the rules of include/tgs_raster.h ("tetrahedral grids"): any device.  It issues the
framework ops the geometry stage's own implementation issues (boolean-mask indexing, ``torch.unique(..., return_inverse=True)`` over every
vertex slot or every edge, stacks and a cat), so on a device it is also the op chain that tools/tet_grid_loop.py times the native calls against.

Also here: the hand-made scene ``odd`` (the other scenes are tests/mt_ref.py's), the fixture's reader and the comparison by bits.
"""
import functools
import os

import numpy as np
import torch

from tests import mt_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tet_grid_fixture.npz")
FIXTURE_SCENES = ("odd", "kuhn_8")
COMPACT_KEYS = ("new_pos", "new_sdf", "new_tets", "new_mask", "new_tet_idx_to_old")
SUBDIV_KEYS = ("new_v", "new_tets", "new_mask", "sub_to_parent")
MARK_KEYS = ("keep_verts_indices", "keep_pos", "keep_sdf", "keep_tets", "keep_tet_idx", "unique_grid_vtx", "new_pos", "new_sdf", "new_tets", "mask_keep_part_in_new_pos")
# the eight sub-tetrahedra over the columns a b c d ab ac ad bc bd cd
A, B, C, D, AB, AC, AD, BC, BD, CD = range(10)
SUB = ((A, AB, AC, AD), (B, BC, AB, BD), (C, AC, BC, CD), (D, AD, CD, BD), (AB, AC, AD, BD), (AB, AC, BD, BC), (CD, AC, BD, AD), (CD, AC, BC, BD))


def selection(sdf, tet, threshold=0.02):
    """-> bool [F]: |mean of the four sdf values| <= threshold, the sum left to right in the dtype of ``sdf``"""
    s = sdf.reshape(-1)[tet.long()]
    return ((((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]) * 0.25).abs() <= threshold


def select_and_remap(tet, keep):
    """the tetrahedra under the bool mask ``keep`` over their own vertices -> (unique_vtx, new_tets, new_tet_idx_to_old)"""
    old = torch.nonzero(keep)[:, 0]
    unique_vtx, inverse = torch.unique(tet.long()[old].reshape(-1), return_inverse=True)
    return unique_vtx, inverse.reshape(-1, 4), old


def compact_tets(pos, sdf, tet, mask=None, threshold=0.02):
    """-> (new_pos, new_sdf, new_tets, new_mask, new_tet_idx_to_old)"""
    with torch.no_grad():
        unique_vtx, new_tets, old = select_and_remap(tet, selection(sdf, tet, threshold))
        return pos[unique_vtx], sdf[unique_vtx], new_tets, None if mask is None else mask[unique_vtx], old


def subdivide_tets(pos, tet, mask=None):
    """pos [N,3], tet [F,4], mask [N,1] or [N] -> (new_v, new_tets, new_mask [N+E,1] float32, sub_to_parent, edges)"""
    N, F, dev = len(pos), len(tet), pos.device
    tet = tet.long()
    if F == 0:
        return pos, tet.reshape(0, 4), None if mask is None else mask.reshape(-1, 1).float(), tet.reshape(0, 4)[:, 0], tet.reshape(0, 4)[:, :2]
    ends = tet[:, torch.tensor(R.EDGES, device=dev).reshape(-1)].reshape(-1, 2)
    pairs = torch.stack([ends.min(-1).values, ends.max(-1).values], -1)
    edges, inverse = torch.unique(pairs, dim=0, return_inverse=True)
    new_v = torch.cat([pos, (pos[edges[:, 0]] + pos[edges[:, 1]]) * 0.5])
    new_mask = None
    if mask is not None:
        m = mask.reshape(-1)
        new_mask = torch.cat([m.float(), ((m[edges[:, 0]] + m[edges[:, 1]]) == 2).float()]).reshape(-1, 1)
    columns = torch.cat([tet, inverse.reshape(-1, 6) + N], 1)
    new_tets = torch.cat([columns[:, list(rows)] for rows in SUB])
    return new_v, new_tets, new_mask, torch.arange(F, device=dev).repeat(8), edges


def mark_part_tets(grid_vertices, level, indices, edit_mask):
    """-> the dict of MARK_KEYS; membership by vertex index"""
    with torch.no_grad():
        f2t = R.marching_tets(grid_vertices, level, indices)["face_to_tet_idx"]
        keep = torch.zeros(len(indices), dtype=torch.bool, device=grid_vertices.device)
        keep[f2t[edit_mask.reshape(-1) == 0]] = True
        level = level.reshape(-1, 1)
        k_vtx, k_tets, k_idx = select_and_remap(indices, keep)
        n_vtx, n_tets, _ = select_and_remap(indices, ~keep)
        member = torch.isin(n_vtx, k_vtx).int().reshape(-1, 1)
        return dict(zip(MARK_KEYS, (k_vtx, grid_vertices[k_vtx], level[k_vtx], k_tets, k_idx, n_vtx, grid_vertices[n_vtx], level[n_vtx], n_tets, member)))


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
T02 = np.float32(0.02)
ABOVE = np.nextafter(T02, np.float32(1.0))
ODD_EXACT_ROWS = (0, 1, 2, 3, 4, 5, 6)                     # rows of ``odd`` whose four values are all +-0.02f or the next float32 above


@functools.lru_cache(maxsize=None)
def odd():
    """26 vertices, 18 rows: descending and permuted indices, a tetrahedron listed twice, one with a repeated vertex, vertices no row uses (4, 22,
    23), a NaN and an infinite sdf, rows of four times exactly 0.02f (kept), of the next float32 above it (dropped) and of -0.02f (kept), and a
    0/1 mask whose edges are of all three kinds"""
    rng = np.random.default_rng(2601)
    sdf = np.array([T02] * 4 + [0.5] + [ABOVE] * 4 + [-T02] * 4 + [np.nan, np.inf, 0.004, -0.006, 0.011, -0.3, 0.25, 0.001, -0.002, 0.0, -1.0, 0.6, -0.013], np.float32)
    tet = [(3, 1, 0, 2), (2, 0, 3, 1), (8, 7, 6, 5), (5, 8, 6, 7), (12, 9, 11, 10), (9, 10, 11, 12), (0, 0, 1, 2),
           (15, 16, 17, 21), (15, 16, 17, 21), (21, 20, 16, 15), (13, 15, 16, 17), (14, 15, 16, 17), (18, 19, 15, 16), (24, 19, 18, 25), (1, 9, 15, 25),
           (3, 12, 20, 16), (24, 24, 19, 19), (25, 18, 2, 10)]
    pos = rng.uniform(0.0, 1.0, (len(sdf), 3))
    s = R._scene(pos, sdf, tet)
    s["mask"] = (np.arange(len(sdf)) % 3 != 0).astype(np.int32)[:, None]
    s["mask"].setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    """a scene of tests/mt_ref.py with a 0/1 vertex mask added (the half-space x < 1/2 of the unjittered grid, so a shell has all three kinds of edge)"""
    if name == "odd":
        return odd()
    s = dict(R.scene(name))
    s["mask"] = (s["pos"][:, :1] < 0.5).astype(np.int32)
    s["mask"].setflags(write=False)
    return s


def tensors(name, device="cpu", column=True):
    s = scene(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    return t(s["pos"]), t(s["sdf"][:, None] if column else s["sdf"]), t(s["tet"]), t(s["mask"])


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def bits(a):
    """an array as something np.array_equal compares exactly: floats by their bits (so NaN positions and payloads count), integers as int64"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()))


@functools.lru_cache(maxsize=None)
def chain(name, threshold):
    """the restatement on the CPU, computed once: compact_tets at ``threshold`` then subdivide_tets of its result, with the mask -> (compact, subdivided)"""
    pos, sdf, tet, mask = tensors(name)
    c = compact_tets(pos, sdf, tet, mask, threshold)
    return c, subdivide_tets(c[0], c[2], c[3])


@functools.lru_cache(maxsize=None)
def whole(name):
    """the restatement's subdivision of a whole scene, with the mask, computed once"""
    pos, _, tet, mask = tensors(name)
    return subdivide_tets(pos, tet, mask)
