"""Mesh normals, edges and the two smoothness losses, restated in torch from the rules of include/tgs_raster.h ("mesh geometry"): any float
dtype, any device, differentiable by plain autograd.  It issues framework ops of the kind the geometry stage's own implementation issues (gathers,
``index_add_``, ``torch.unique(dim=0)``), so on a device it is also the op chain that tools/mesh_geom_loop.py times the native calls against.

Also here: the scenes of the tests (meshes from tests/mt_ref.py, ``traps``, ``umbrella``), the per-row figures the tests' conditions are stated
in, the comparison that leaves non-finite rows to a row-wise check, and the fixture's reader.
"""
import functools
import os

import numpy as np
import torch

from tests import mesh_grad_ref as G
from tests import mt_ref as MT

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mesh_geom_fixture.npz")
FIXTURE_SCENES = ("cases16", "fan", "kuhn_8", "traps")
SCENES = FIXTURE_SCENES + ("kuhn_32", "kuhn_32_small", "umbrella")
NORMAL_EPS, COSINE_EPS = 1e-20, 1e-8
KUHN_32_SMALL_DEFAULT_ROWS = 5          # rows of kuhn_32_small whose float64 squared sum is at or below the threshold
F64, F32 = torch.float64, torch.float32


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
def edges_of(faces):
    """[F,3] integer -> [E,2] int64: the distinct (min, max) pairs of the 3 F sides, ascending; a pair (i, i) is kept"""
    f = faces.long()
    sides = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    pairs = torch.stack([sides.min(-1).values, sides.max(-1).values], -1)
    return torch.unique(pairs, dim=0) if len(pairs) else pairs


def normal_sums(v_pos, faces):
    """-> [V,3]: per vertex the sum of the normals cross(v1 - v0, v2 - v0) of the faces it is a corner of"""
    f = faces.long()
    p0, p1, p2 = v_pos[f[:, 0]], v_pos[f[:, 1]], v_pos[f[:, 2]]
    n = torch.linalg.cross(p1 - p0, p2 - p0, dim=-1)
    s = torch.zeros_like(v_pos)
    for c in range(3):
        s = s.index_add(0, f[:, c], n)
    return s


def vertex_normals(v_pos, faces):
    s = normal_sums(v_pos, faces)
    default = torch.tensor([0.0, 0.0, 1.0], dtype=v_pos.dtype, device=v_pos.device)
    s = torch.where((s * s).sum(-1, keepdim=True) > NORMAL_EPS, s, default)
    return s / torch.sqrt((s * s).sum(-1, keepdim=True).clamp(min=NORMAL_EPS))


def cosine(x, y):
    """each row divided by max(|row|, eps), then the dot product: what torch.cosine_similarity evaluates (tests/test_mesh_geom_ref.py compares)"""
    xn, yn = torch.linalg.vector_norm(x, dim=-1, keepdim=True), torch.linalg.vector_norm(y, dim=-1, keepdim=True)
    return ((x / xn.clamp_min(COSINE_EPS)) * (y / yn.clamp_min(COSINE_EPS))).sum(-1)


def normal_consistency(v_nrm, edges):
    return (1.0 - cosine(v_nrm[edges[:, 0]], v_nrm[edges[:, 1]])).mean()


def laplacian(v_pos, edges):
    """the mean row norm of the uniform Laplacian of the distinct adjacency; a pair (i, i) adds -1 and +1 to the diagonal: nothing"""
    e = edges[edges[:, 0] != edges[:, 1]]
    d = v_pos[e[:, 0]] - v_pos[e[:, 1]]
    rows = torch.zeros_like(v_pos).index_add(0, e[:, 0], d).index_add(0, e[:, 1], -d)
    return torch.linalg.vector_norm(rows, dim=1).mean()


def mesh_normal_consistency(v_pos, faces, edges=None):
    return normal_consistency(vertex_normals(v_pos, faces), edges_of(faces) if edges is None else edges)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _mesh(v_pos, faces):
    m = dict(v_pos=np.ascontiguousarray(v_pos, np.float32), faces=np.ascontiguousarray(faces, np.int64))
    for a in m.values():
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def traps():
    """by hand: an isolated vertex (11), faces (i,i,i) and (i,i,j), a duplicated face, and two faces on three vertices of their own (12, 13, 14) with
    opposite winding, whose normals cancel exactly in any order"""
    rng = np.random.default_rng(2207)
    v = np.zeros((15, 3))
    v[0] = (0.0, 0.0, 0.4)
    ang = np.arange(8) * (2 * np.pi / 8)
    v[1:9] = np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    v[9], v[10], v[11] = (0.0, 0.0, -0.7), (2.0, 0.3, 0.1), (5.0, 5.0, 5.0)
    v[12:15] = ((3.0, 0.0, 0.0), (4.0, 0.0, 0.5), (3.0, 1.0, 0.25))
    v[:11] += rng.uniform(-0.05, 0.05, (11, 3))
    f = [(0, 1 + i, 1 + (i + 1) % 8) for i in range(8)] + [(9, 1 + (i + 1) % 8, 1 + i) for i in range(0, 8, 2)]
    f += [(1, 10, 2), (3, 3, 3), (4, 4, 5), (10, 10, 2), (0, 3, 4), (12, 13, 14), (12, 14, 13), (6, 9, 6)]          # (0, 3, 4) is face 2 again
    assert len(f) != 3 and f[2] == f[-4]
    return _mesh(v, f)


@functools.lru_cache(maxsize=None)
def umbrella():
    """one apex with 300 faces around it: an incidence run and a max-end list longer than a wave"""
    rng = np.random.default_rng(2208)
    n = 300
    ang = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(5 * ang)], 1) + rng.uniform(-0.003, 0.003, (n, 3))
    v = np.concatenate([ring, [[0.0, 0.0, 0.5]]])                             # the apex has the largest index: its edges are all on the max side
    return _mesh(v, [(n, i, (i + 1) % n) for i in range(n)])


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(v_pos [V,3] float32, faces [F,3] int64), read-only"""
    if name == "traps":
        return traps()
    if name == "umbrella":
        return umbrella()
    base = "kuhn_32" if name == "kuhn_32_small" else name
    r64, r32 = MT.reference(base)
    v = r32["verts"].astype(np.float32)                                      # what a float32 marching_tets hands on
    return _mesh(v / 16.0 if name == "kuhn_32_small" else v, r64["faces"])


def tensors(name, dtype, device="cpu", grad=False):
    m = scene(name)
    return torch.tensor(m["v_pos"], device=device).to(dtype).requires_grad_(grad), torch.tensor(m["faces"], device=device)


@functools.lru_cache(maxsize=None)
def row_figures(name):
    """-> (the float64 squared length of every vertex's normal sum, |sum n_f| / sum |n_f| with 1 where nothing is summed)"""
    v, f = tensors(name, F64)
    s = normal_sums(v, f)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ln = torch.linalg.cross(p1 - p0, p2 - p0, dim=-1).norm(dim=-1)
    tot = torch.zeros(len(v), dtype=F64)
    for c in range(3):
        tot = tot.index_add(0, f[:, c], ln)
    sq = (s * s).sum(-1)
    ratio = torch.where(tot > 0, sq.sqrt() / tot.clamp(min=1e-300), torch.ones_like(tot))
    return sq.numpy(), ratio.numpy()


def left_out(name):
    """the rows that take no part in a comparison: kuhn_32_small's rows within a factor 2 of the threshold"""
    sq, _ = row_figures(name)
    return (sq > 0.5 * NORMAL_EPS) & (sq < 2.0 * NORMAL_EPS) if name == "kuhn_32_small" else np.zeros(len(sq), bool)


def upstream(name, tag):
    """[V,3] float32 for the normals: ``random``, or ``one_row`` (a vertex in the middle); zero on the rows that are left out"""
    V = len(scene(name)["v_pos"])
    g = np.zeros((V, 3), np.float32)
    if tag == "random":
        g[:] = np.random.default_rng(900 + V).uniform(-1.0, 1.0, (V, 3))
    else:
        g[V // 2] = (1.0, -0.5, 0.25)
    g[left_out(name)] = 0.0
    return g


SCALAR_UPSTREAM = np.float32(0.75)


@functools.lru_cache(maxsize=None)
def reference(name, what, tag="random"):
    """what in normals / consistency / consistency_of_normals / laplacian -> per dtype (float64, float32) the pair (value, gradient) as float64
    numpy arrays, read-only.  consistency: of the float32 normals as data, gradient to them; consistency_of_normals: the chain from v_pos."""
    res = []
    for f in (F64, F32):
        v, faces = tensors(name, f, grad=True)
        e = edges_of(faces)
        if what == "normals":
            out = vertex_normals(v, faces)
            (out * torch.tensor(upstream(name, tag)).to(f)).sum().backward()
            leaf = v
        elif what == "consistency":
            leaf = torch.tensor(reference(name, "normals")[1][0].astype(np.float32)).to(f).requires_grad_(True)
            out = normal_consistency(leaf, e)
            (out * float(SCALAR_UPSTREAM)).backward()
        else:
            out = mesh_normal_consistency(v, faces, e) if what == "consistency_of_normals" else laplacian(v, e)
            (out * float(SCALAR_UPSTREAM)).backward()
            leaf = v
        pair = (out.detach().double().numpy().copy(), leaf.grad.double().numpy().copy())
        for a in pair:
            a.setflags(write=False)
        res.append(pair)
    return tuple(res)


def rules_zero_rows(name):
    """the rows whose ``v_pos`` gradient through the normals is zero by the rules, whatever arrives: every face the vertex is a corner of (none, for
    an isolated vertex) has three default rows as its corners"""
    m = scene(name)
    sq, _ = row_figures(name)
    default = ~(sq > NORMAL_EPS)
    dead_face = default[m["faces"]].all(axis=1)
    live = np.zeros(len(sq), bool)
    live[m["faces"][~dead_face].reshape(-1)] = True
    return ~live


def compare(what, got, ref64, ref32, skip=None, exact_zero=None):
    """rows: the non-finite rows are the reference's, row-wise, and every other row (but ``skip``) is within tests/mesh_grad_ref.py's ``check_bars``.
    A row that the rules leave at zero is zero in the restatement at both precisions, and must be exactly zero.  A row that is zero in float64 and
    not in float32 is zero by cancellation (cases16: a lone triangle's three normals are equal and the consistency's gradient cancels, to the last
    bit in some rows): no arithmetic but the reference's own reproduces that, so such a row is held to the same 4 eta and not to equality.
    Where both precisions cancel to the last bit (cases16 has such a triangle) the caller names the rows that are zero by the rules, ``exact_zero``."""
    got, ref64, ref32 = (np.asarray(a).reshape(-1, 3) if np.ndim(a) == 2 else np.asarray(a).reshape(1, 1) for a in (got, ref64, ref32))
    bad = ~np.isfinite(ref64).all(axis=1)
    assert np.array_equal(~np.isfinite(got).all(axis=1), bad), (what, int(bad.sum()), int((~np.isfinite(got).all(axis=1)).sum()))
    keep = ~bad & np.isfinite(ref32).all(axis=1)
    if skip is not None:
        keep &= ~skip
    if not keep.any():
        return 0.0, 0.0
    by_cancellation = keep & ~(ref64 != 0).any(axis=1) & ((ref32 != 0).any(axis=1) if exact_zero is None else ~exact_zero)
    if by_cancellation.any():
        eta = float(np.abs(ref32 - ref64)[keep].max())
        assert np.abs(got[by_cancellation]).max() <= 4.0 * eta, (what, float(np.abs(got[by_cancellation]).max()), eta)
        keep &= ~by_cancellation
    return G.check_bars(what, got[keep], ref64[keep], ref32[keep])


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))
