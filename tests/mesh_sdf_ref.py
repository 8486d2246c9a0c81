"""The mesh signed distance restated in numpy float64, by brute force over all faces (include/tgs_raster.h, "mesh signed distance";
youreditableavatar_amd/csrc/tgs_mesh_sdf.hpp): the exact point-to-triangle distance with the lowest face and its closest point, the three ray parities
with the tie rule, the majority.  Every product and sum is written as the native code writes it, one operation at a time (numpy does not fuse).

``query(vertices, faces, points)`` -> dict(sdf, dist, face, closest, inside, parity, flag): ``dist`` is the distance in float64, ``sdf`` the signed
distance rounded once to float32, ``parity`` [N,3] the parities along x, y, z, and ``flag`` the per-point MARGIN FLAG: set when some edge value with
``0 < |E| < 2^-40 (|t1| + |t2|)`` occurs (t1, t2 its two products), or when a counted face has a height within ``2^-30`` of ``p_k`` -- where the
sign of a rounded number decides ``inside``, and two correct evaluations may disagree.  A point at distance exactly 0 carries no flag: it is inside
by the rule for ``d == 0``, whatever its parities are, so no rounded sign decides anything there."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mesh_sdf_fixture.npz")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _segment(p, a, b):
    ab = b - a
    den = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0.0, _dot(p - a, ab) / den, 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    return a + t[..., None] * ab


def _dist2(p, c):
    d = p - c
    return _dot(d, d)


def _segments(p, a, b, c):
    best = _segment(p, a, b)
    bd = _dist2(p, best)
    for u, v in ((b, c), (c, a)):
        cand = _segment(p, u, v)
        d = _dist2(p, cand)
        take = d < bd
        bd = np.where(take, d, bd)
        best = np.where(take[..., None], cand, best)
    return best


def closest_on_triangle(p, a, b, c):
    """p, a, b, c: float64 arrays [...,3] that broadcast -> the closest point of each triangle to each point [...,3]"""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)                                                       # (y z - z y, z x - x z, x y - y x): the same three expressions
    flat = (n[..., 0] == 0.0) & (n[..., 1] == 0.0) & (n[..., 2] == 0.0)
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    s = (va + vb) + vc
    col = lambda x: x[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        e_ab = a + col(d1 / (d1 - d3)) * ab
        e_ac = a + col(d2 / (d2 - d6)) * ac
        e_bc = b + col((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
        v, w = vb / s, vc / s
        inner = (a + ab * col(v)) + ac * col(w)
    seg = _segments(p, a, b, c)
    conds = [flat, (d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
             (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0), ~(s > 0.0)]
    picks = [seg, a, b, e_ab, c, e_ac, e_bc, seg]
    out = inner
    for cond, pick in zip(reversed(conds), reversed(picks)):                     # the first condition that holds wins
        out = np.where(col(cond), pick, out)
    return out


def point_triangle_distance(p, a, b, c):
    """-> the distance [...] in float64"""
    p = np.asarray(p, np.float64)
    return np.sqrt(_dist2(p, closest_on_triangle(p, np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))))


def _sign(x):
    return (x > 0.0).astype(np.int64) - (x < 0.0).astype(np.int64)


def _edge(ia, xa, ya, ib, xb, yb, pa, pb):
    """one edge of every face [F] against every point [N,1] -> (the oriented value [N,F], the oriented sign, the margin flag)"""
    fwd = ia < ib
    ua, ub, va, vb = np.where(fwd, xa, xb), np.where(fwd, ya, yb), np.where(fwd, xb, xa), np.where(fwd, yb, ya)
    t1, t2 = (va - ua) * (pb - ub), (vb - ub) * (pa - ua)
    E = t1 - t2
    s = _sign(E)
    tie = np.where(-(vb - ub) != 0.0, _sign(-(vb - ub)), _sign(va - ua))
    s = np.where(s == 0, tie, s)
    same = ia == ib
    flag = (E != 0.0) & (np.abs(E) < 2.0 ** -40 * (np.abs(t1) + np.abs(t2))) & ~same
    return np.where(same, 0.0, np.where(fwd, E, -E)), np.where(same, 0, np.where(fwd, s, -s)), flag


def crossings(vertices, faces, points, k):
    """-> (crosses [N,F] bool: the ray from each point along +k crosses each face, the margin flag [N])"""
    a, b = (k + 1) % 3, (k + 2) % 3
    i = [faces[:, c].astype(np.int64) for c in range(3)]
    v = [vertices[i[c]].astype(np.float64) for c in range(3)]
    pa, pb, pk = (points[:, x].astype(np.float64)[:, None] for x in (a, b, k))
    e, s, flags = [], [], np.zeros(len(points), bool)
    for c in range(3):
        n = (c + 1) % 3
        ec, sc, fc = _edge(i[c], v[c][:, a], v[c][:, b], i[n], v[n][:, a], v[n][:, b], pa, pb)
        e.append(ec), s.append(sc)
        flags |= fc.any(axis=1)
    total = (e[0] + e[1]) + e[2]
    contained = (s[0] != 0) & (s[0] == s[1]) & (s[0] == s[2]) & (total != 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = ((e[0] * v[2][:, k] + e[1] * v[0][:, k]) + e[2] * v[1][:, k]) / total
    counted = contained & (h > pk)
    flags |= (counted & (np.abs(h - pk) < 2.0 ** -30)).any(axis=1)
    return counted, flags


def query(vertices, faces, points, chunk=None):
    vertices, faces, points = np.asarray(vertices, np.float32), np.asarray(faces), np.asarray(points, np.float32)
    N, F = len(points), len(faces)
    chunk = chunk or max(1, (1 << 21) // max(F, 1))
    out = dict(sdf=np.empty(N, np.float32), dist=np.empty(N), face=np.empty(N, np.int32), closest=np.empty((N, 3), np.float32), inside=np.empty(N, bool),
               parity=np.empty((N, 3), bool), flag=np.empty(N, bool))
    a, b, c = (vertices[faces[:, k].astype(np.int64)].astype(np.float64)[None] for k in range(3))
    for lo in range(0, N, chunk):
        pts = points[lo:lo + chunk]
        sl = slice(lo, lo + len(pts))
        ok = np.isfinite(pts).all(axis=1)
        p = np.where(ok[:, None], pts, 0.0).astype(np.float64)
        cl = closest_on_triangle(p[:, None, :], a, b, c)                         # [n,F,3]
        d2 = _dist2(p[:, None, :], cl)
        face = np.argmin(d2, axis=1)                                           # the first of the least: the lowest face
        rows = np.arange(len(p))
        best = d2[rows, face]
        par, flag = np.empty((len(p), 3), bool), np.zeros(len(p), bool)
        for k in range(3):
            cross, fl = crossings(vertices, faces, p.astype(np.float32), k)
            par[:, k] = cross.sum(axis=1) % 2 == 1
            flag |= fl
        dist = np.sqrt(best)
        inside = (par.sum(axis=1) >= 2) | (best == 0.0)
        mag = dist.astype(np.float32)
        out["dist"][sl] = np.where(ok, dist, np.nan)
        out["sdf"][sl] = np.where(ok, np.where(best == 0.0, np.float32(0.0), np.where(inside, mag, -mag)), np.float32(np.nan))
        out["face"][sl] = np.where(ok, face, -1)
        out["closest"][sl] = np.where(ok[:, None], cl[rows, face].astype(np.float32), np.float32(np.nan))
        out["inside"][sl] = ok & inside
        out["parity"][sl] = par & ok[:, None]
        out["flag"][sl] = flag & ok & (best != 0.0)
    return out


# ---- the scenes the tests share ---------------------------------------------------------------------------------------------------------
def cube(lo=-0.5, hi=0.5, lid=True):
    """the axis-aligned cube [lo, hi]^3 as 12 triangles, outward; ``lid=False`` leaves the two triangles of the +z face out"""
    v = np.array([[(hi if i & 1 else lo), (hi if i & 2 else lo), (hi if i & 4 else lo)] for i in range(8)], np.float32)
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)] + ([(4, 5, 7, 6)] if lid else [])
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return v, f


def two_cubes():
    """[-0.5, 0.5]^3 and the same cube moved by (0.5, 0.25, 0.125): they overlap"""
    v, f = cube()
    return np.concatenate([v, v + np.array([0.5, 0.25, 0.125], np.float32)]), np.concatenate([f, f + 8])


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, np.array(f, np.int32)


def icosphere(levels, dent=0.0):
    """a unit icosphere of 20 * 4^levels faces; ``dent`` pushes the vertices around +z towards the centre"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    if dent:
        w = np.clip((v[:, 2] - 0.6) / 0.4, 0.0, 1.0)
        v = v * (1.0 - dent * w * w * (3.0 - 2.0 * w))[:, None]
    return v.astype(np.float32), np.array(f, np.int32)


# every scene of the CPU and the GPU tests: name -> (vertices, faces)
SCENES = {
    "triangle": lambda: (cube()[0], cube()[1][:1]),
    "tetrahedron": tetrahedron,
    "cube": lambda: cube(0.0, 1.0),
    "lidless_cube": lambda: cube(0.0, 1.0, lid=False),
    "two_cubes": two_cubes,
    "cube_and_flat_faces": lambda: (np.concatenate([cube(0.0, 1.0)[0], np.array([[0.5, 0.0, 0.0]], np.float32)]),
                                    np.concatenate([cube(0.0, 1.0)[1], np.array([[0, 8, 1], [0, 0, 1], [3, 3, 3]], np.int32)])),
    "icosphere_20": lambda: icosphere(0),
    "icosphere_1280": lambda: icosphere(3, dent=0.3),
    "one_leaf": lambda: (icosphere(0)[0], icosphere(0)[1][:4]),
    "one_leaf_and_one": lambda: (icosphere(0)[0], icosphere(0)[1][:5]),
}


def scene_points(v, n=300, seed=11):
    """seeded points around the mesh, points of a dyadic grid (ties), points on vertices, a NaN and an infinity"""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0) - 0.5, v.max(0) + 0.5
    grid = np.array([[x, y, z] for x in (-0.5, 0.0, 0.25, 0.5, 1.0) for y in (-0.5, 0.0, 0.5, 1.0, 1.5) for z in (-0.25, 0.0, 0.5, 1.0)], np.float32)
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]], np.float32)
    return np.concatenate([rng.uniform(lo, hi, (n, 3)).astype(np.float32), grid, v[:8], bad])


def ulp32(x):
    """the spacing of float32 at |x| (the smallest subnormal at 0)"""
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def check_bars(vertices, faces, points, ref, sdf, face, closest, inside, what=""):
    """one implementation's answers against the restatement's (``ref``: what ``query`` returned for these points) under the four bars -> the number of
    points with the margin flag.  Distance: |sdf| within one float32 ulp of the restatement's distance rounded to float32 (both are double
    evaluations with about 1e-15 relative error: after one rounding they differ by at most one ulp).  Face: the returned face, put through the
    restatement's own point-to-triangle function, gives that same distance within one ulp.  Closest point: | ||p - closest|| - d | <= sqrt(3) 2^-24
    max|coordinate| (each coordinate of closest is rounded to float32).  Inside: equal wherever the margin flag is not set; at most 0.5 % carry it."""
    vertices, points = np.asarray(vertices, np.float32), np.asarray(points, np.float32)
    sdf, face, closest, inside = np.asarray(sdf), np.asarray(face), np.asarray(closest), np.asarray(inside).astype(bool)
    assert sdf.dtype == np.float32 and closest.dtype == np.float32 and sdf.shape == (len(points),) and closest.shape == (len(points), 3), what
    ok = np.isfinite(points).all(axis=1)
    assert np.isnan(sdf[~ok]).all() and (face[~ok] == -1).all() and not inside[~ok].any() and np.isnan(closest[~ok]).all(), what
    assert np.array_equal(ok, ref["face"] >= 0)
    points, sdf, face, closest, inside = points[ok], sdf[ok], face[ok], closest[ok], inside[ok]
    dist, flag, want_inside = ref["dist"][ok], ref["flag"][ok], ref["inside"][ok]
    want = dist.astype(np.float32)
    err = np.abs(np.abs(sdf).astype(np.float64) - want.astype(np.float64))
    print(f"{what}: {len(points)} points, |sdf| off by at most {float((err / ulp32(want)).max()) if len(points) else 0.0:.2f} ulp", end="")
    assert (err <= ulp32(want)).all(), what
    assert ((face >= 0) & (face < len(faces))).all(), what
    tri = vertices[np.asarray(faces)[face].astype(np.int64)].astype(np.float64)
    via = point_triangle_distance(points, tri[:, 0], tri[:, 1], tri[:, 2]).astype(np.float32)
    assert (np.abs(via.astype(np.float64) - want.astype(np.float64)) <= ulp32(want)).all(), what
    off = np.abs(np.linalg.norm(points.astype(np.float64) - closest.astype(np.float64), axis=1) - dist)
    bound = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(vertices).max())
    print(f", closest off by at most {float(off.max()) if len(points) else 0.0:.3g} (bound {bound:.3g})", end="")
    assert (off <= bound).all(), what
    print(f", {int(flag.sum())} margin flags ({100.0 * flag.mean() if len(points) else 0.0:.2f} %)")
    assert flag.sum() <= 0.005 * len(points), what
    assert np.array_equal(inside[~flag], want_inside[~flag]), what
    assert np.array_equal(sdf, np.where(dist == 0.0, np.float32(0.0), np.where(inside, np.abs(sdf), -np.abs(sdf)))), what     # the sign is inside's
    assert not np.signbit(sdf[dist == 0.0]).any() and inside[dist == 0.0].all(), what
    return int(flag.sum())


def load_fixture():
    """-> (vertices, faces, points, the restatement's outputs as ``query`` returns them, the recorded count of margin flags)"""
    z = np.load(FIXTURE)
    return z["vertices"], z["faces"], z["points"], {k[4:]: z[k] for k in z.files if k.startswith("out_")}, int(z["flagged"])
