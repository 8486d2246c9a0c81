"""GPU: the exclusive scan of csrc/tgs_runs.hpp, one text compiled into three translation units, at the smallest sizes where it gains a level or a tile
is partial.  A tile is 2048 elements, so the scanned array has 2048 (one full tile), 2049 (a second tile of one element: two levels), 4097 (a third
tile of one element) or 2048^2 + 1 = 4 194 305 elements (three levels).  Each translation unit is reached through its own calls:

  tgs_mesh_geom.hip      ``mesh_topology``: three scans over V + 1 (mg_carve)
  tgs_marching_tets.hip  ``marching_tets``, forward (one scan over N + 1, mt_carve) and backward (two over N + 1, mt_grad_carve)
  tgs_tet_grid.hip       ``subdivide_tets``: two scans over N + 1 (tg_subdiv_carve); ``compact_tets``: its longest scan is over the bitmap's
                         (N + 63) / 64 + 1 words (tg_compact_carve), so it has the cases 2048, 2049 and 4097 at N = 131 008, 131 072 and 262 144

The mesh is a handful of faces or tetrahedra over the vertices that sit on the tiles' boundaries (``corners``), everything else is unused.  Expected
values come from the CPU restatements (tests/mesh_geom_ref.py, tests/mt_ref.py, tests/tet_ref.py) on the same arrays; integers and the subdivision's
midpoints are exact, marching tetrahedra's vertices and gradients are held to the bars of tests/test_gpu_marching_tets.py (4 eta; check_bars)."""
import numpy as np
import pytest
import torch

from tests import mesh_geom_ref as MG
from tests import mesh_grad_ref as G
from tests import mt_ref as MT
from tests import tet_ref as T

pytestmark = pytest.mark.gpu
TILE = 2048
LENGTHS = (TILE, TILE + 1, 2 * TILE + 1, TILE * TILE + 1)
WORD_LENGTHS = (TILE, TILE + 1, 2 * TILE + 1)


def corners(n, step=1):
    """the vertices below ``n`` whose element of the scanned array is the first, the last, in the middle of the first tile or next to a tile's boundary
    (``step`` vertices to an element)"""
    marks = (0, 1, TILE // 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE * TILE - 1, TILE * TILE)
    return sorted({v for m in marks for v in (m * step, m * step + step - 1) if v < n} | {n - 2, n - 1})


def simplices(n, k, step=1):
    """a handful of rows of ``k`` corners each: every window of k neighbours, one row spread over all of them and one over both ends; every second
    row turned over -> int64 [*, k]"""
    c = corners(n, step)
    rows = [tuple(c[i:i + k]) for i in range(len(c) - k + 1)] + [tuple(c[i] for i in np.linspace(0, len(c) - 1, k).astype(int)), (c[0], c[-1], c[1], c[-2])[:k]]
    rows = list(dict.fromkeys(rows))
    return torch.tensor([r[::-1] if i % 2 else r for i, r in enumerate(rows)], dtype=torch.int64)


def values(n, seed, lo=-1.0, hi=1.0, cols=3):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, (n, cols)).astype(np.float32))


def words(t):
    return t.detach().cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("length", LENGTHS)
def test_mesh_topology(length):
    import youreditableavatar_amd.mesh_geom as mg
    V = length - 1
    faces = simplices(V, 3)
    assert len(faces) >= 4 and int(faces.min()) == 0 and int(faces.max()) == V - 1
    topo = mg.mesh_topology(faces.cuda(), V)
    want, flat, F = MG.edges_of(faces).numpy(), faces.numpy().reshape(-1), len(faces)
    assert topo.num_edges == len(want) < 3 * F and np.array_equal(topo.edges.cpu().numpy(), want)      # (some sides are shared)
    ends = lambda of: np.concatenate([np.cumsum(np.bincount(of, minlength=V)), [len(of)]])             # element V: the total, which no cursor moves
    assert np.array_equal(words(topo.inc), np.argsort(flat, kind="stable"))
    assert np.array_equal(words(topo.inc_end), ends(flat))
    assert np.array_equal(words(topo.edge_end), ends(want[:, 0]))
    assert np.array_equal(words(topo.max_end), ends(want[:, 1]))
    assert np.array_equal(words(topo.max_list), np.argsort(want[:, 1], kind="stable"))


def grid_scene(N):
    """pos, sdf, tet: a handful of tetrahedra over the corners, each with corners on both sides of the surface"""
    pos, tet = values(N, 11 + N), simplices(N, 4)
    sdf = values(N, 12 + N, 0.1, 1.0, 1)[:, 0]
    inside = torch.zeros(N, dtype=torch.bool)
    inside[torch.tensor(corners(N)[::2])] = True
    return pos, torch.where(inside, sdf, -sdf), tet


@pytest.mark.parametrize("length", LENGTHS)
def test_marching_tets_forward_and_backward(length):
    import youreditableavatar_amd.marching_tets as mt
    N = length - 1
    pos, sdf, tet = grid_scene(N)
    ref = {}
    for f in (torch.float64, torch.float32):
        p, s = pos.to(f, copy=True).requires_grad_(True), sdf.to(f, copy=True).requires_grad_(True)
        out = MT.marching_tets(p, s, tet)
        if f == torch.float64:
            g = values(len(out["verts"]), 13 + N)
        (out["verts"] * g.to(f)).sum().backward()
        ref[f] = out, p.grad.double().numpy(), s.grad.double().numpy()[:, None]
    want, v32 = ref[torch.float64][0], ref[torch.float32][0]["verts"].detach().double().numpy()
    assert int(want["valid_tets"].sum()) >= 3 and len(want["verts"]) >= 6
    p, s = pos.cuda().requires_grad_(True), sdf.cuda().requires_grad_(True)
    got = mt.marching_tets(p, s, tet.cuda())
    for k in ("valid_tets", "interp_v", "faces", "face_to_tet_idx"):
        assert np.array_equal(got[k].cpu().numpy(), want[k].numpy()), (length, k)
    v64, verts = want["verts"].detach().numpy(), got["verts"].detach().cpu().numpy()
    eta, err = float(np.abs(v32 - v64).max()), float(np.abs(verts - v64).max())
    print(f"scan of {length}: verts eta {eta:.3g} err {err:.3g}")
    assert verts.dtype == np.float32 and err <= 4.0 * eta, (length, err, eta)
    got["verts"].backward(g.cuda())
    G.check_bars(f"scan of {length} dL_dpos", p.grad.cpu().numpy(), ref[torch.float64][1], ref[torch.float32][1])
    G.check_bars(f"scan of {length} dL_dsdf", s.grad.cpu().numpy().reshape(-1, 1), ref[torch.float64][2], ref[torch.float32][2])


@pytest.mark.parametrize("length", LENGTHS)
def test_subdivide_tets(length):
    import youreditableavatar_amd.tet_grid as tg
    N = length - 1
    pos, _, tet = grid_scene(N)
    mask = torch.zeros(N, 1, dtype=torch.int32)
    mask[torch.tensor(corners(N)[::3])] = 1
    want = T.subdivide_tets(pos, tet, mask)
    assert 6 <= len(want[4]) < 6 * len(tet)                                      # (some edges are shared)
    got = tg.subdivide_tets(pos.cuda(), tet.cuda(), mask.cuda())
    for k, g, w in zip(T.SUBDIV_KEYS + ("edges",), got, want):
        T.assert_same(g, w, f"scan of {length}: {k}")


@pytest.mark.parametrize("length", WORD_LENGTHS)
def test_compact_tets(length):
    import youreditableavatar_amd.tet_grid as tg
    N = (length - 1) * 64                                                        # (N + 63) / 64 + 1 words
    c, other = corners(N, 64), 5
    assert (N + 63) // 64 + 1 == length and other not in c
    tet = torch.cat([simplices(N, 4, 64), torch.tensor([[c[0], other, c[2], c[-1]], [c[-1], c[3], other, c[1]]])])
    pos, sdf = values(N, 21 + N), values(N, 22 + N, -0.01, 0.01, 1)
    sdf[other] = 1.0                                                             # the two rows that hold it are dropped: a mean of 0.25
    mask = torch.arange(N, dtype=torch.int64)[:, None] % 5
    want = T.compact_tets(pos, sdf, tet, mask)
    assert len(want[4]) == len(tet) - 2 and int(tet[want[4]].max()) == N - 1 and int(tet[want[4]].min()) == 0
    got = tg.compact_tets(pos.cuda(), sdf.cuda(), tet.cuda(), mask.cuda())
    for k, g, w in zip(T.COMPACT_KEYS, got, want):
        T.assert_same(g, w, f"scan of {length} words: {k}")
