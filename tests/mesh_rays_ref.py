"""The mesh ray casting restated in numpy float64, by brute force over all faces (include/tgs_raster.h, "mesh ray casting";
youreditableavatar_amd/csrc/tgs_mesh_rays.hpp): the shear of Woop, Benthin and Wald, the three edge values, the candidate test with exact zeros on both
sides, det, t, the rule for a zero cross product, the least t with the lowest face, the uvs and the unit normal.  Every product and sum is written as the
native code writes it, one operation at a time (numpy does not fuse).

``cast(vertices, faces, rays)`` -> dict(t, t_hit, face, uv, normal, flag): ``t`` is the hit parameter in float64 (+inf on a miss), ``t_hit`` that number
rounded once to float32, and ``flag`` the per-ray MARGIN FLAG, set where the sign of a rounded number or the order of two rounded numbers decides the answer
and two correct evaluations may disagree:
  * for a face with ``t >= 0`` that is not above the best ``t`` by more than ``2^-30`` relative (every such face, when nothing is hit), some ``U``, ``V`` or
    ``W`` has ``0 < |value| < 2^-40 (|p1| + |p2|)``, p1 and p2 its two products; or ``0 < |det| < 2^-40 (|U| + |V| + |W|)``;
  * two different faces' hits are within ``2^-40`` relative of the least ``t`` without being equal.
Exact zeros and exact ties carry no flag: the tie rule decides them.  (A face with ``t < 0`` is no hit whatever its signs say, so it sets no flag.)"""
import functools

import numpy as np

from tests import mesh_sdf_ref as S

ulp32 = S.ulp32
MISS_ID = -1


def _take(a, k):
    """a [n,...,3], k [n] -> the component k[n] of every row of ray n"""
    idx = k.reshape((len(k),) + (1,) * (a.ndim - 1))
    return np.take_along_axis(a, np.broadcast_to(idx, a.shape[:-1] + (1,)), axis=-1)[..., 0]


def setup(rays):
    """rays [n,6] float32 -> (valid [n], o, d in float64 (an invalid ray replaced by a harmless one), kx, ky, kz, Sx, Sy, Sz)"""
    rays = np.asarray(rays, np.float32)
    valid = np.isfinite(rays).all(axis=1) & (rays[:, 3:] != 0.0).any(axis=1)
    r = np.where(valid[:, None], rays, np.array([0, 0, 0, 0, 0, 1], np.float32)).astype(np.float64)
    o, d = r[:, :3], r[:, 3:]
    kz = np.argmax(np.abs(d), axis=1)                                          # the first of the largest: the lowest axis on a tie
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    dz = _take(d, kz)
    kx, ky = np.where(dz < 0.0, ky, kx), np.where(dz < 0.0, kx, ky)
    return valid, o, d, kx, ky, kz, _take(d, kx) / dz, _take(d, ky) / dz, 1.0 / dz


def _shear(P, o, kx, ky, kz, Sx, Sy, Sz):
    A = P - o[:, None, :]
    az = _take(A, kz)
    return _take(A, kx) - Sx[:, None] * az, _take(A, ky) - Sy[:, None] * az, Sz[:, None] * az


def _cross(a, b, c):
    e, g = b - a, c - a
    return np.stack([e[..., 1] * g[..., 2] - e[..., 2] * g[..., 1], e[..., 2] * g[..., 0] - e[..., 0] * g[..., 2], e[..., 0] * g[..., 1] - e[..., 1] * g[..., 0]], axis=-1)


def pairs(ray, a, b, c):
    """the pair function: every ray of ``ray`` (what ``setup`` returned, without ``valid``) against the faces (a, b, c), float64 [1 or n, F, 3] ->
    dict(hit [n,F], t, U, V, W, det, margin: some value or det inside its margin)"""
    o = ray[0]
    Ax, Ay, Az = _shear(a, o, *ray[2:])
    Bx, By, Bz = _shear(b, o, *ray[2:])
    Cx, Cy, Cz = _shear(c, o, *ray[2:])
    u1, u2, v1, v2, w1, w2 = Cx * By, Cy * Bx, Ax * Cy, Ay * Cx, Bx * Ay, By * Ax
    U, V, W = u1 - u2, v1 - v2, w1 - w2
    cand = ~(((U < 0.0) | (V < 0.0) | (W < 0.0)) & ((U > 0.0) | (V > 0.0) | (W > 0.0)))
    det = (U + V) + W
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = ((U * Az + V * Bz) + W * Cz) / det
    flat = (_cross(a, b, c) == 0.0).all(axis=-1)
    hit = cand & (det != 0.0) & (t >= 0.0) & np.isfinite(t) & ~flat
    small = lambda x, p, q: (x != 0.0) & (np.abs(x) < 2.0 ** -40 * (np.abs(p) + np.abs(q)))
    margin = small(U, u1, u2) | small(V, v1, v2) | small(W, w1, w2) | ((det != 0.0) & (np.abs(det) < 2.0 ** -40 * ((np.abs(U) + np.abs(V)) + np.abs(W))))
    return dict(hit=hit, t=t, U=U, V=V, W=W, det=det, margin=margin & ~flat)


def unit_normal(a, b, c):
    n = _cross(a, b, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        return n / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]


def cast(vertices, faces, rays, chunk=None):
    vertices, faces, rays = np.asarray(vertices, np.float32), np.asarray(faces), np.asarray(rays, np.float32).reshape(-1, 6)
    N, F = len(rays), len(faces)
    chunk = chunk or max(1, (1 << 20) // max(F, 1))
    out = dict(t=np.full(N, np.inf), t_hit=np.full(N, np.inf, np.float32), face=np.full(N, MISS_ID, np.int32), uv=np.zeros((N, 2), np.float32),
               normal=np.zeros((N, 3), np.float32), flag=np.zeros(N, bool))
    a, b, c = (vertices[faces[:, k].astype(np.int64)].astype(np.float64)[None] for k in range(3))
    for lo in range(0, N, chunk):
        valid, *ray = setup(rays[lo:lo + chunk])
        n = len(valid)
        sl, rows = slice(lo, lo + n), np.arange(n)
        p = pairs(ray, a, b, c)
        tt = np.where(p["hit"], p["t"], np.inf)
        face = np.argmin(tt, axis=1)                                           # the first of the least: the lowest face
        best = tt[rows, face]
        hit = valid & np.isfinite(best)
        with np.errstate(invalid="ignore"):
            near = (p["t"] >= 0.0) & (p["t"] <= (best + 2.0 ** -30 * np.abs(best))[:, None])          # best == inf: every face with t >= 0
            close = p["hit"] & (tt != best[:, None]) & (np.abs(tt - best[:, None]) <= 2.0 ** -40 * np.abs(best)[:, None])
        flag = (near & p["margin"]).any(axis=1) | close.any(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = np.stack([p["V"][rows, face] / p["det"][rows, face], p["W"][rows, face] / p["det"][rows, face]], axis=1)
        nrm = unit_normal(a[0, face], b[0, face], c[0, face])
        out["t"][sl] = np.where(hit, best, np.inf)
        out["t_hit"][sl] = np.where(hit, best, np.inf).astype(np.float32)
        out["face"][sl] = np.where(hit, face, MISS_ID)
        out["uv"][sl] = np.where(hit[:, None], uv, 0.0).astype(np.float32)
        out["normal"][sl] = np.where(hit[:, None], nrm, 0.0).astype(np.float32)
        out["flag"][sl] = flag & valid
    return out


def one_face(vertices, faces, rays, face):
    """the pair function for ray n against the face ``face[n]`` alone -> (hit [n], t [n]); an invalid ray hits nothing"""
    vertices, faces, rays = np.asarray(vertices, np.float32), np.asarray(faces), np.asarray(rays, np.float32).reshape(-1, 6)
    valid, *ray = setup(rays)
    a, b, c = (vertices[faces[face, k].astype(np.int64)].astype(np.float64)[:, None, :] for k in range(3))
    p = pairs(ray, a, b, c)
    return p["hit"][:, 0] & valid, p["t"][:, 0]


# ---- the scenes and the rays the tests share --------------------------------------------------------------------------------------------------
INVALID_RAYS = np.array([[np.nan, 0, 0, 0, 0, 1], [0.5, 0.5, -2, 0, np.inf, 1], [0.5, 0.5, -2, 0, 0, 0]], np.float32)      # a NaN origin, an infinite direction, d == 0


def scene_rays(v, n=300, seed=23):
    """seeded origins within four diameters of the mesh's centre, aimed at seeded points of its box, with directions of seeded length; a dyadic grid of axis
    rays (exact ties on the cubes); rays through the first 8 vertices; the three invalid rays.  Every |o_k| stays below 64 times the largest |coordinate|,
    the range the header gives for the slab test."""
    v = np.asarray(v, np.float32)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    centre, diam = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    way = rng.normal(size=(n, 3))
    o = centre + way / np.linalg.norm(way, axis=1, keepdims=True) * (rng.uniform(0.0, 4.0, (n, 1)) * diam)
    d = (rng.uniform(lo, hi, (n, 3)) - o) * rng.uniform(0.25, 2.0, (n, 1))
    seeded = np.concatenate([o, d], axis=1).astype(np.float32)
    G = (-0.5, 0.0, 0.25, 0.5, 1.0)
    grid = []
    for k in range(3):
        for p in G:
            for q in G:
                o3, d3 = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                o3[k], o3[(k + 1) % 3], o3[(k + 2) % 3], d3[k] = -2.0, p, q, 2.0 if (p + q) > 0.5 else 1.0
                grid.append(o3 + d3)
    eye = (centre + np.array([1.5, -1.25, 2.0]) * diam).astype(np.float32)
    # (the direction is scaled by 0.7 before it is rounded: with d == v - eye exactly, the faces around the vertex give hits a rounding apart, which is
    # what the margin flag is for, and half of such rays carry it)
    through = np.concatenate([np.broadcast_to(eye, (len(v[:8]), 3)), (v[:8].astype(np.float64) - eye.astype(np.float64)) * 0.7], axis=1)
    rays = np.concatenate([seeded, np.array(grid, np.float32), through.astype(np.float32), INVALID_RAYS])
    assert float(np.abs(rays[:-3, :3]).max()) <= 64.0 * float(np.abs(v).max())
    return rays


def scene_names():
    return sorted(S.SCENES) + ["body"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (vertices, faces, rays, the restatement's answer): computed once per process, shared by every test, never written to"""
    if name == "body":
        v, f = S.load_fixture()[:2]
    else:
        v, f = S.SCENES[name]()
    rays = scene_rays(v)
    ref = cast(v, f, rays)
    for a in (v, f, rays, *ref.values()):
        a.setflags(write=False)
    return v, f, rays, ref


# ---- the closed-form rays of the cube and the icosphere -----------------------------------------------------------------------------------------
def cube_tie_rays():
    """rays aimed exactly at a shared diagonal, at an edge and at a corner of the unit cube [0,1]^3 (dyadic numbers: every edge value involved is exact)
    -> (rays [n,6], the exact t [n])"""
    rays = [[0.5, 0.5, -2, 0, 0, 1],           # the -z face's diagonal (faces 0 and 1 share the edge 0-3: x == y), t = 2
            [0.25, 0.25, 3, 0, 0, -2],         # the +z face's diagonal from above, t = 1
            [0.5, -1, -1, 0, 1, 1],            # the cube's edge y = z = 0, from the outside across it, t = 1
            [-1, -1, 0.5, 1, 1, 0],            # the vertical edge x = y = 0, from the outside along the diagonal, t = 1
            [-1, -1, -1, 1, 1, 1],             # the corner (0,0,0) along the space diagonal, t = 1
            [2, 2, 2, -0.5, -0.5, -0.5],       # the corner (1,1,1), t = 2
            [2.5, -1.5, -1.5, -0.5, 0.5, 0.5]] # the corner (1,0,0), t = 3
    return np.array(rays, np.float32), np.array([2, 1, 1, 1, 1, 2, 3], np.float64)


def icosphere_seam_rays(v, f):
    """from the centre towards every vertex and towards every edge midpoint (rounded to float32) -> rays [V + E, 6]"""
    v, f = np.asarray(v, np.float32), np.asarray(f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    mid = ((v[e[:, 0]].astype(np.float64) + v[e[:, 1]].astype(np.float64)) / 2).astype(np.float32)
    d = np.concatenate([v, mid])
    return np.concatenate([np.zeros_like(d), d], axis=1)


# ---- the bars ---------------------------------------------------------------------------------------------------------------------------------------
def check_bars(vertices, faces, rays, ref, t_hit, face, uv, normal, what=""):
    """one implementation's answers against the restatement's (``ref``: what ``cast`` returned for these rays) -> the number of rays with the margin flag.

    t_hit: within one float32 ulp of the restatement's t rounded to float32 (both are double evaluations of the same expressions, rounded once: the
    argument of mesh_sdf_ref.check_bars).  Face, and hit or miss: equal wherever the flag is not set; where it is set, the returned face, put through the
    restatement's own pair function, is a hit whose t is within one ulp of the returned t_hit.  uv and normal components: within 2^-23, one float32 ulp at
    magnitude 1, of the restatement's for the same face.  At most 0.5 % of the rays may carry the flag (a condition on the scene, not a measurement).

    Geometric closure: X = o + t_hit d and Y = (1 - u - v) v0 + u v1 + v v2, evaluated in float64 from the float32 outputs, satisfy
        |X - Y| <= 2^-24 |t| |d|  +  2^-23 sqrt(3) m  +  2^-40 (|t| |d| + |o| + m),        m the mesh's largest |coordinate|.
    Derivation.  In double, before the outputs are rounded, the two points agree up to the double arithmetic: U, V, W of a hit have one sign, so det is
    their sum without cancellation and the weights U/det, V/det, W/det carry a few 2^-53 of relative error; the sheared coordinates carry 2^-52 |P - o|;
    and sum_i weight_i (Ax_i, Ay_i) = 0 is an identity in the computed sheared coordinates, so t is the weighted mean of the Az_i the same weights give.
    Together far below 2^-40 (|t||d| + |o| + m), the third term.  Rounding t to float32 moves X by at most 2^-24 |t| |d| (half an ulp is at most 2^-24
    relative).  Rounding u and v, both in [0, 1] where half an ulp is at most 2^-25, moves Y by at most 2^-25 (|v1 - v0| + |v2 - v0|), and an edge is at most
    the box's diagonal 2 sqrt(3) m: 2^-23 sqrt(3) m."""
    vertices, faces, rays = np.asarray(vertices, np.float32), np.asarray(faces), np.asarray(rays, np.float32).reshape(-1, 6)
    t_hit, face, uv, normal = np.asarray(t_hit).reshape(-1), np.asarray(face).reshape(-1).astype(np.int64), np.asarray(uv).reshape(-1, 2), np.asarray(normal).reshape(-1, 3)
    N = len(rays)
    assert t_hit.dtype == np.float32 and uv.dtype == np.float32 and normal.dtype == np.float32 and len(t_hit) == len(face) == len(uv) == len(normal) == N, what
    face = np.where(face == 0xFFFFFFFF, -1, face)                                 # (uint32 ids of the numpy route)
    valid, flag = setup(rays)[0], ref["flag"]
    hit, want_hit = face >= 0, ref["face"] >= 0
    assert not hit[~valid].any() and not want_hit[~valid].any(), what
    assert (face[hit] < len(faces)).all(), what
    assert np.isposinf(t_hit[~hit]).all() and not uv[~hit].any() and not normal[~hit].any(), what                # miss rows
    assert np.array_equal(hit[~flag], want_hit[~flag]) and np.array_equal(face[~flag], ref["face"][~flag]), what
    both = hit & want_hit
    err = np.abs(t_hit[both].astype(np.float64) - ref["t_hit"][both].astype(np.float64))
    print(f"{what}: {N} rays, {int(hit.sum())} hits, t_hit off by at most {float((err / ulp32(ref['t_hit'][both])).max()) if both.any() else 0.0:.2f} ulp", end="")
    assert (err <= ulp32(ref["t_hit"][both])).all(), what
    odd = flag & hit
    if odd.any():
        ok, t = one_face(vertices, faces, rays[odd], face[odd])
        assert ok.all() and (np.abs(t.astype(np.float32).astype(np.float64) - t_hit[odd].astype(np.float64)) <= ulp32(t_hit[odd])).all(), what
    same = both & (face == ref["face"])
    duv, dn = np.abs(uv[same].astype(np.float64) - ref["uv"][same]), np.abs(normal[same].astype(np.float64) - ref["normal"][same])
    print(f", uv off by {float(duv.max()) if same.any() else 0.0:.3g}, normal by {float(dn.max()) if same.any() else 0.0:.3g} (bar {2.0 ** -23:.3g})", end="")
    assert (duv <= 2.0 ** -23).all() and (dn <= 2.0 ** -23).all(), what
    o, d, t = rays[hit, :3].astype(np.float64), rays[hit, 3:].astype(np.float64), t_hit[hit].astype(np.float64)
    tri = vertices[faces[face[hit]].astype(np.int64)].astype(np.float64)
    u, w = uv[hit, 0].astype(np.float64)[:, None], uv[hit, 1].astype(np.float64)[:, None]
    X, Y = o + t[:, None] * d, ((1.0 - u - w) * tri[:, 0] + u * tri[:, 1]) + w * tri[:, 2]
    m, reach = float(np.abs(vertices).max()), np.abs(t) * np.linalg.norm(d, axis=1)
    bound = 2.0 ** -24 * reach + 2.0 ** -23 * np.sqrt(3.0) * m + 2.0 ** -40 * (reach + np.linalg.norm(o, axis=1) + m)
    gap = np.linalg.norm(X - Y, axis=1)
    print(f", closure at most {float((gap / bound).max()) if hit.any() else 0.0:.3f} of its bound", end="")
    assert (gap <= bound).all(), what
    nn = np.linalg.norm(normal[hit].astype(np.float64), axis=1)
    assert (np.abs(nn - 1.0) <= 3 * 2.0 ** -24).all(), what                         # a unit vector whose three components were rounded
    print(f", {int(flag.sum())} margin flags ({100.0 * flag.mean() if N else 0.0:.2f} %)")
    assert flag.sum() <= 0.005 * N, what
    return int(flag.sum())
