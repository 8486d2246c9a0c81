"""Marching tetrahedra, restated in torch from the rules of include/tgs_raster.h ("marching tetrahedra"): any float dtype, any device,
differentiable by plain autograd.  It issues the framework ops the geometry stage's own implementation issues (boolean-mask indexing, a
``torch.unique(dim=0, return_inverse=True)`` over six edges per surface tetrahedron, masks summed into sizes), so on a device it is also the
op chain that tools/marching_tets_loop.py times the native call against.

Also here: the scenes of the tests (``cases16``, ``fan``, ``kuhn(n)``), the closed-manifold property, and the fixture's reader.
"""
import functools
import itertools
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mt_fixture.npz")
KEYS = ("verts", "faces", "face_to_tet_idx", "valid_tets", "interp_v")
FIXTURE_SCENES = ("cases16", "fan", "kuhn_8")

# a tetrahedron's six edges as pairs of its corners, in the order the rules number them
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# per case code sum_k occ_k 2^k: the triangles, every corner the crossing of the edge between two corners of the tetrahedron
CASES = (
    "",
    "02 01 03",
    "13 01 12",
    "02 13 03 | 02 12 13",
    "12 02 23",
    "03 12 01 | 03 23 12",
    "02 13 01 | 02 23 13",
    "13 03 23",
    "13 23 03",
    "13 02 01 | 13 23 02",
    "12 03 01 | 12 23 03",
    "02 12 23",
    "13 02 03 | 13 12 02",
    "12 01 13",
    "03 01 02",
    "",
)


def _tables():
    number = {f"{i}{j}": k for k, (i, j) in enumerate(EDGES)}
    table = np.zeros((16, 6), np.int64)
    count = np.zeros(16, np.int64)
    for code, text in enumerate(CASES):
        corners = [number[c] for c in text.replace("|", " ").split()]
        table[code, :len(corners)] = corners
        count[code] = len(corners) // 3
    return torch.from_numpy(table), torch.from_numpy(count)


def vertices_of(pos, sdf, interp_v):
    """the mesh vertices on the crossing edges ``interp_v`` [M,2]: w_a = (-sdf[b]) / D, w_b = sdf[a] / D, D = sdf[a] + (-sdf[b])"""
    a, b = interp_v[:, 0], interp_v[:, 1]
    sa, nb = sdf[a], -sdf[b]
    D = sa + nb
    return pos[a] * (nb / D)[:, None] + pos[b] * (sa / D)[:, None]


def marching_tets(pos, sdf, tet):
    """pos [N,3], sdf [N] or [N,1] (one float dtype), tet [F,4] integer -> the dict of KEYS"""
    dev = pos.device
    sdf = sdf.reshape(-1)
    tet = tet.long()
    table, count = (t.to(dev) for t in _tables())
    with torch.no_grad():
        occ = sdf > 0
        occ4 = occ[tet.reshape(-1)].reshape(-1, 4)
        inside = occ4.sum(-1)
        valid = (inside > 0) & (inside < 4)
        vt, vocc = tet[valid], occ4[valid].long()
        code = (vocc * (2 ** torch.arange(4, device=dev))).sum(-1)
        corners = torch.tensor(EDGES, device=dev)
        ends = vt[:, corners.reshape(-1)].reshape(-1, 2)
        edges = torch.stack([ends.min(-1).values, ends.max(-1).values], -1)
        unique, inverse = torch.unique(edges, dim=0, return_inverse=True) if len(edges) else (edges, edges[:, 0])
        crossing = occ[unique[:, 0]] != occ[unique[:, 1]]
        row = torch.full((len(unique),), -1, dtype=torch.long, device=dev)
        row[crossing] = torch.arange(int(crossing.sum()), device=dev)
        edge_row = row[inverse].reshape(-1, 6)
        interp_v = unique[crossing]
    verts = vertices_of(pos, sdf, interp_v)
    n_tri = count[code]
    one, two = n_tri == 1, n_tri == 2
    faces = torch.cat([torch.gather(edge_row[one], 1, table[code[one]][:, :3]).reshape(-1, 3),
                       torch.gather(edge_row[two], 1, table[code[two]]).reshape(-1, 3)])
    which = torch.nonzero(valid)[:, 0]
    return dict(verts=verts, faces=faces, face_to_tet_idx=torch.cat([which[one], which[two].repeat_interleave(2)]), valid_tets=valid, interp_v=interp_v)


def run(scene, dtype, device="cpu"):
    """a scene's float32 arrays evaluated in ``dtype`` -> the dict of KEYS as numpy arrays (verts in float64)"""
    out = marching_tets(torch.tensor(scene["pos"], device=device).to(dtype), torch.tensor(scene["sdf"], device=device).to(dtype), torch.tensor(scene["tet"], device=device))
    return {k: (v.double() if k == "verts" else v).cpu().numpy() for k, v in out.items()}


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _scene(pos, sdf, tet):
    s = dict(pos=np.asarray(pos, np.float32), sdf=np.asarray(sdf, np.float32), tet=np.asarray(tet, np.int64))
    for a in s.values():
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def cases16():
    """16 disjoint tetrahedra, tetrahedron f with case code f, the 64 vertex indices permuted (so raw edges occur as (hi, lo) too)"""
    rng = np.random.default_rng(1601)
    perm = rng.permutation(64)
    tet = perm.reshape(16, 4)
    assert (tet[:, :-1] > tet[:, 1:]).any() and (tet[:, :-1] < tet[:, 1:]).any()
    pos, sdf = np.zeros((64, 3)), np.zeros(64)
    for f in range(16):
        for k in range(4):
            v = tet[f, k]
            pos[v] = np.array([f % 4, f // 4, 0.0]) + rng.uniform(0.0, 0.8, 3)
            sdf[v] = rng.uniform(0.1, 1.0) * (1.0 if f >> k & 1 else -1.0)
    return _scene(pos, sdf, tet)


@functools.lru_cache(maxsize=None)
def fan():
    """two fans of ten tetrahedra around the shared edges (0, 1) and (1, 12) over one ring of ten vertices, with an exact-zero corner, a NaN
    corner on a valid tetrahedron, a tetrahedron listed twice and one with a repeated vertex"""
    rng = np.random.default_rng(1602)
    ring = list(range(2, 12))
    tet = [(0, 1, ring[i], ring[(i + 1) % 10]) for i in range(10)] + [(ring[(i + 1) % 10], 12, 1, ring[i]) for i in range(10)]
    tet += [tet[2], (0, 0, ring[1], ring[2]), tet[13]]
    ang = np.arange(10) * (2 * np.pi / 10)
    pos = np.concatenate([[[0, 0, 0.5], [0, 0, -0.5]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1), [[0, 0, -1.5]]]) + rng.uniform(-0.1, 0.1, (13, 3))
    sdf = np.concatenate([[0.6, -0.4], np.where(np.arange(10) % 5 < 3, -1.0, 1.0) * rng.uniform(0.2, 0.9, 10), [0.7]])
    sdf[ring[3]] = 0.0                                      # outside, and the vertex on an edge to it lies on it
    sdf[ring[7]] = np.nan                                   # outside; the vertices on its crossing edges are NaN
    return _scene(pos, sdf, tet)


@functools.lru_cache(maxsize=None)
def kuhn(n):
    """an n^3-cube grid of the unit cube, six tetrahedra per cube: one per axis permutation, the monotone path from the cube's low to its high
    corner, re-ordered to positive volume.  pos: the grid jittered by +-0.2 cell; sdf = 0.37 - |x - 1/2| plus noise of +-0.3 cell."""
    rng = np.random.default_rng(3200 + n)
    m = n + 1
    idx = lambda i, j, k: (i * m + j) * m + k
    i, j, k = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"))
    unit = np.eye(3, dtype=np.int64)
    tets = []
    for perm in itertools.permutations(range(3)):
        at = np.stack([i, j, k], 1)
        path = [idx(*at.T)]
        for axis in perm:
            at = at + unit[axis]
            path.append(idx(*at.T))
        even = np.linalg.det(unit[list(perm)].astype(float)) > 0
        tets.append(np.stack(path if even else [path[0], path[1], path[3], path[2]], 1))
    tet = np.stack(tets, 1).reshape(-1, 4)                  # cube by cube
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3) / n
    pos = (g + rng.uniform(-0.2, 0.2, g.shape) / n).astype(np.float32)
    sdf = 0.37 - np.linalg.norm(pos.astype(np.float64) - 0.5, axis=1) + rng.uniform(-0.3, 0.3, len(g)) / n
    return _scene(pos, sdf, tet)


def scene(name):
    return cases16() if name == "cases16" else fan() if name == "fan" else kuhn(int(name.split("_")[1]))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (the restatement in float64, in float32), read-only numpy dicts, computed once"""
    out = tuple(run(scene(name), f) for f in (torch.float64, torch.float32))
    for d in out:
        for a in d.values():
            a.setflags(write=False)
    return out


# ---- properties ------------------------------------------------------------------------------------------------------------------------
def manifold_counts(faces, n_verts):
    """-> dict: directed edges that occur more than once, undirected edges not shared by exactly two faces, the Euler characteristic"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, dc = np.unique(d, axis=0, return_counts=True)
    _, uc = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return dict(directed_repeated=int((dc != 1).sum()), undirected_not_two=int((uc != 2).sum()), euler=int(n_verts - len(uc) + len(f)),
                unused_verts=int(n_verts - len(np.unique(f))))


def min_abs_sdf_on_crossing(scene_, interp_v):
    return float(np.abs(scene_["sdf"][np.asarray(interp_v).reshape(-1)]).min())
