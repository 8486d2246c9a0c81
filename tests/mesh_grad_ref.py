"""Torch float64 CPU restatement of the mesh rasterizer's gradient rules (include/tgs_raster.h, "mesh rasterizer: gradients").

The integer decisions are tests/mesh_ref.py's and tests/mesh_aa_ref.py's (snapping, topology, pixel IDs: imported); the per-pair decisions of
antialias, which tests/mesh_aa_ref.py does not expose, are recomputed here by the same steps (``aa_pairs``) and checked against its output in
tests/test_mesh_grad_ref.py.  The smooth parts are written in torch, so autograd gives the gradients; nothing here differentiates by hand.
Every smooth function takes the GATHERED vertex rows (one copy per pixel or pair): called on ``pos[index]`` autograd scatters for us (the chain
test), called on a leaf copy its ``.grad`` holds the per-pixel contributions, whose largest magnitude B and largest count per destination n
give the fixed-point term of the header.  The same code run in float32 gives the noise eta.  Nothing here looks at the code under test."""
import functools

import numpy as np
import torch

from tests import mesh_aa_ref as A
from tests import mesh_ref as M

GRAD_FRAC = 34                     # include/tgs_raster.h: a contribution becomes llrint(c 2^(34 - e)) with 2^(e-1) <= B < 2^e
RAST_SCENES = ("grid_97x61", "coarse_200x150", "offscreen_40x24", "sphere_256", "fullscreen_512", "patch_97x61", "flaps_64x48", "ball_96", "tinypatch_128")
INTERP_SCENES = ("hand_33x17", "grid_97x61", "sphere_256", "tinypatch_128", "fullscreen_512")
AA_GRAD_SCENES = A.NON_VACUOUS + ("sphere_256",)
CHANNELS = A.CHANNELS


scene, scene_rast = A.scene, A.scene_rast             # (tests/mesh_aa_ref.py serves tests/mesh_ref.py's scenes too: the CPU reference's image, read-only)


def upstream(name, shape, tag, smooth=False):
    """a seeded upstream gradient, float32: uniform in [-1, 1], or (``smooth``) a few low-frequency waves over the image plus a channel ramp"""
    rng = np.random.default_rng(sum(ord(ch) for ch in name + tag) * 16 + shape[-1])
    if not smooth:
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    H, W, C = shape
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.zeros(shape)
    for c in range(C):
        fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 6.28)
        out[..., c] = np.sin(6.28 * (fx * x + fy * y) + ph) + 0.3 * (c + 1)
    return out.astype(np.float32)


def _t(a, dtype):
    return torch.tensor(np.asarray(a, np.float32), dtype=torch.float32).to(dtype)


def fixed_point_term(B, n):
    """the header's bound on what fixed-point rounding adds to an element that n contributions reach: n 2^(e - 35), 2^(e-1) <= B < 2^e.  B is
    the reference's largest |contribution|, widened by 2^-20 for the kernel's own measurement of it (fp32-rounded)."""
    if B == 0.0 or n == 0:
        return 0.0
    _, e = np.frexp(float(B) * (1.0 + 2.0 ** -20))
    return float(n) * 2.0 ** (int(e) - GRAD_FRAC - 1)


# ---- interpolate ---------------------------------------------------------------------------------------------------------------------
def covered(rast, tri, V):
    """-> (flat indices of the pixels with an ID in [1, F] whose triangle's indices lie in [0, V), their vertex indices [n,3])"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    r = np.asarray(rast, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        hit = (r[:, 3] >= 1.0) & (r[:, 3] <= float(len(tri)))
    pix = np.nonzero(hit)[0]
    vid = tri[r[pix, 3].astype(np.int64) - 1] if len(tri) else np.zeros((0, 3), np.int64)
    good = ((vid >= 0) & (vid < V)).all(axis=1)
    return pix[good], vid[good]


def interpolate_torch(A3, uv):
    """A3 [n,3,C] the three vertices' attribute rows, uv [n,2] -> [n,C]"""
    u, v = uv[:, 0:1], uv[:, 1:2]
    return u * A3[:, 0] + v * A3[:, 1] + (1.0 - u - v) * A3[:, 2]


def interpolate_grads(dtype, attr, rast, tri, g):
    """attr [V,C], rast [H,W,4], g [H,W,C] (float32 arrays) -> dict: d_attr [V,C], d_rast [H,W,4] (float64 arrays, evaluated in ``dtype``),
    B (the bound of the dL_dattr scatter: max |g|, the three weights lie in [0, 1]), n (the largest number of pixels that reach one row)"""
    attr, rast, g = np.asarray(attr, np.float32), np.asarray(rast, np.float32), np.asarray(g, np.float32)
    V, C = attr.shape
    H, W = rast.shape[:2]
    pix, vid = covered(rast, tri, V)
    at = _t(attr, dtype).requires_grad_(True)
    uv = _t(rast.reshape(-1, 4)[pix][:, :2], dtype).requires_grad_(True)
    vt = torch.from_numpy(vid)
    out = interpolate_torch(at[vt.reshape(-1)].reshape(-1, 3, C), uv)
    (out * _t(g.reshape(-1, C)[pix], dtype)).sum().backward()
    d_rast = np.zeros((H * W, 4))
    d_rast[pix, :2] = uv.grad.double().numpy()
    d_attr = at.grad.double().numpy() if at.grad is not None else np.zeros((V, C))
    n = int(np.bincount(vid.reshape(-1), minlength=1).max()) if len(pix) else 0
    return dict(d_attr=d_attr, d_rast=d_rast.reshape(H, W, 4), B=float(np.abs(g).max()) if g.size else 0.0, n=n)


# ---- rasterize -----------------------------------------------------------------------------------------------------------------------
def uv_torch(P, i, j, W, H):
    """tests/mesh_ref.py's ``float_part`` in torch, in the same order: P [n,3,4] the winning triangle's clip-space vertices per pixel, i, j the
    pixel -> u, v (clamped, divided by max(u + v, 1)) and the unclamped u0 = q0/d, v0 = q1/d"""
    f = P.dtype
    x, y, w = P[..., 0], P[..., 1], P[..., 3]
    sx, sy, iw = (x / w * 0.5 + 0.5) * W, (y / w * 0.5 + 0.5) * H, 1.0 / w
    e1x, e1y, e2x, e2y = sx[:, 1] - sx[:, 0], sy[:, 1] - sy[:, 0], sx[:, 2] - sx[:, 0], sy[:, 2] - sy[:, 0]
    inv = 1.0 / (e1x * e2y - e1y * e2x)
    px, py = (i.to(f) + 0.5) - sx[:, 0], (j.to(f) + 0.5) - sy[:, 0]
    b1 = (px * e2y - py * e2x) * inv
    b2 = (e1x * py - e1y * px) * inv
    b0 = (1.0 - b1) - b2
    q0, q1, q2 = b0 * iw[:, 0], b1 * iw[:, 1], b2 * iw[:, 2]
    d = (q0 + q1) + q2
    u0, v0 = q0 / d, q1 / d
    uc, vc = u0.clamp(0.0, 1.0), v0.clamp(0.0, 1.0)                               # (torch: derivative 1 inside and at the bounds, 0 outside)
    s = (uc + vc).clamp(min=1.0)
    assert uc.dtype == f
    return uc / s, vc / s, u0, v0


def uv_ambiguous(pos, tri, rast):
    """-> (bool [H,W]: covered pixels whose unclamped u0, v0 or u0 + v0 lie within 4x the fp32 evaluation noise of a clamp bound, the number of
    covered pixels).  The noise is the largest |fp32 - fp64| of that quantity over the covered pixels."""
    pos, rast = np.asarray(pos, np.float32).reshape(-1, 4), np.asarray(rast, np.float32)
    H, W = rast.shape[:2]
    pix, vid = covered(rast, tri, len(pos))
    amb = np.zeros(H * W, bool)
    if len(pix) == 0:
        return amb.reshape(H, W), 0
    i, j = torch.from_numpy(pix % W), torch.from_numpy(pix // W)
    with torch.no_grad():
        _, _, u64, v64 = uv_torch(_t(pos[vid], torch.float64), i, j, W, H)
        _, _, u32, v32 = uv_torch(_t(pos[vid], torch.float32), i, j, W, H)
    near = np.zeros(len(pix), bool)
    for q64, q32, bounds in ((u64, u32, (0.0, 1.0)), (v64, v32, (0.0, 1.0)), (u64 + v64, u32 + v32, (1.0,))):
        eta = float((q32.double() - q64).abs().max())
        for b in bounds:
            near |= ((q64 - b).abs() <= 4.0 * eta).numpy()
    amb[pix] = near
    return amb.reshape(H, W), len(pix)


def rasterize_grads(dtype, pos, tri, rast, g):
    """pos [V,4], rast [H,W,4], g [H,W,4] (float32 arrays; channels 2 and 3 of g are ignored) -> dict: d_pos [V,4] float64 array evaluated in
    ``dtype``, B the largest |per-pixel contribution|, n the largest number of pixels that reach one vertex"""
    pos, rast, g = np.asarray(pos, np.float32).reshape(-1, 4), np.asarray(rast, np.float32), np.asarray(g, np.float32)
    H, W = rast.shape[:2]
    V = len(pos)
    pix, vid = covered(rast, tri, V)
    if len(pix) == 0:
        return dict(d_pos=np.zeros((V, 4)), B=0.0, n=0)
    P = _t(pos[vid], dtype).requires_grad_(True)
    u, v, _, _ = uv_torch(P, torch.from_numpy(pix % W), torch.from_numpy(pix // W), W, H)
    gp = _t(g.reshape(-1, 4)[pix], dtype)
    (u * gp[:, 0] + v * gp[:, 1]).sum().backward()
    d_pos = torch.zeros((V, 4), dtype=dtype).index_add_(0, torch.from_numpy(vid.reshape(-1)), P.grad.reshape(-1, 4))
    return dict(d_pos=d_pos.double().numpy(), B=float(P.grad.abs().max()), n=int(np.bincount(vid.reshape(-1)).max()))


# ---- antialias -----------------------------------------------------------------------------------------------------------------------
def aa_pairs(rast, pos, tri, topo):
    """The forward's decisions for every pair that contributes (the steps of tests/mesh_aa_ref.py's ``antialias``, which keeps them to itself)
    -> dict of arrays over those pairs: R, O (flat index of the receiver and of the other pixel), sign (+1 where a > 0, -1 where a < 0), va, vb
    (the exit edge's vertex indices), Px, Py, ux, uy (the pixel that shows the triangle and the step to the other one, snapped units), horiz,
    t (the snapped crossing position E / -D, float64)."""
    rast = np.asarray(rast, np.float32)
    H, W = rast.shape[:2]
    pos, tri = np.asarray(pos, np.float32).reshape(-1, 4), np.asarray(tri, np.int64).reshape(-1, 3)
    V, F = len(pos), len(tri)
    keys = ("R", "O", "sign", "va", "vb", "Px", "Py", "ux", "uy", "horiz", "t")
    if F == 0 or V == 0:
        return {k: np.zeros(0, bool if k == "horiz" else np.float64 if k == "t" else np.int64) for k in keys}
    topo = np.asarray(topo, np.int64)
    ids, z = A.pixel_ids(rast).reshape(-1), rast[..., 2].reshape(-1)
    flat = np.arange(H * W).reshape(H, W)
    p1 = np.concatenate([flat[:, :-1].reshape(-1), flat[:-1, :].reshape(-1)])
    p2 = np.concatenate([flat[:, 1:].reshape(-1), flat[1:, :].reshape(-1)])
    horiz = np.concatenate([np.ones(H * (W - 1), bool), np.zeros((H - 1) * W, bool)])
    keep = ids[p1] != ids[p2]
    p1, p2, horiz = p1[keep], p2[keep], horiz[keep]
    id1, id2, z1, z2 = ids[p1], ids[p2], z[p1], z[p2]
    with np.errstate(invalid="ignore"):
        nearer = (z1 < z2) | (~(z2 < z1) & (id1 < id2))
    first = np.where((id1 != 0) & (id2 != 0), nearer, id1 != 0)
    P, Q = np.where(first, p1, p2), np.where(first, p2, p1)
    tid = np.where(first, id1, id2)
    live = (tid >= 1) & (tid <= F)
    T = np.clip(tid - 1, 0, F - 1)
    vid = tri[T]
    live &= ((vid >= 0) & (vid < V)).all(axis=1)
    vid = np.clip(vid, 0, V - 1)
    X, Y, ok, _, _ = M.snap(pos, W, H)
    live &= ok[vid].all(axis=1)
    vx, vy = X[vid], Y[vid]
    Ar = (vx[:, 1] - vx[:, 0]) * (vy[:, 2] - vy[:, 0]) - (vx[:, 2] - vx[:, 0]) * (vy[:, 1] - vy[:, 0])
    live &= Ar != 0
    s = np.sign(Ar)
    Px, Py = 256 * (P % W) + 128, 256 * (P // W) + 128
    ux, uy = 256 * (Q % W - P % W), 256 * (Q // W - P // W)
    n = len(P)
    kexit, Ee, De = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64)
    for k in (2, 1, 0):                                                           # descending: the first qualifying k is what remains
        a, b = k, (k + 1) % 3
        dX, dY = vx[:, b] - vx[:, a], vy[:, b] - vy[:, a]
        D = s * (dX * uy - dY * ux)
        E = s * (dX * (Py - vy[:, a]) - dY * (Px - vx[:, a]))
        extent = np.where(horiz, (np.minimum(vy[:, a], vy[:, b]) <= Py) & (Py <= np.maximum(vy[:, a], vy[:, b])),
                          (np.minimum(vx[:, a], vx[:, b]) <= Px) & (Px <= np.maximum(vx[:, a], vx[:, b])))
        q = (D < 0) & (E >= 0) & (E <= -D) & extent
        kexit, Ee, De = np.where(q, k, kexit), np.where(q, E, Ee), np.where(q, D, De)
    go = live & (kexit >= 0)
    ke = np.maximum(kexit, 0)
    rows = np.arange(n)
    o = topo[T, ke]
    ia, ib = vid[rows, ke], vid[rows, (ke + 1) % 3]
    oc = np.clip(o, 0, V - 1)
    Eo = s * ((X[ib] - X[ia]) * (Y[oc] - Y[ia]) - (Y[ib] - Y[ia]) * (X[oc] - X[ia]))
    go &= (o == A.NONE) | (o == A.MANY) | ((o >= 0) & (o < V) & ok[oc] & (Eo >= 0))
    t64 = Ee.astype(np.float64) / (-De).astype(np.float64)
    a32 = t64.astype(np.float32) - np.float32(0.5)
    go &= a32 != 0
    sel = np.nonzero(go)[0]
    pos_a = a32[sel] > 0
    vals = dict(R=np.where(pos_a, Q[sel], P[sel]), O=np.where(pos_a, P[sel], Q[sel]), sign=np.where(pos_a, 1, -1), va=ia[sel], vb=ib[sel], Px=Px[sel], Py=Py[sel],
                ux=ux[sel], uy=uy[sel], horiz=horiz[sel], t=t64[sel])
    return vals


def aa_torch(color, PA, PB, pr, W, H, real=False):
    """color [H*W,C], PA, PB [n,4] the exit edges' vertices per pair, pr = aa_pairs(...) -> out [H*W,C].
    The crossing position on the real-valued screen coordinates is t~ = E(P) / (-D).  ``real``: the blend weight IS |t~ - 0.5| (the function
    the finite differences perturb).  Otherwise its VALUE is the forward's -- the snapped t, rounded to ``color``'s precision as the kernel
    rounds it -- and its derivative is t~'s: the rule's "derivative of snapping taken as 1"."""
    f = color.dtype
    R, O = torch.from_numpy(pr["R"]), torch.from_numpy(pr["O"])
    sign, Px, Py, ux, uy = (torch.from_numpy(pr[k]).to(f) for k in ("sign", "Px", "Py", "ux", "uy"))
    Xa, Ya = (PA[:, 0] / PA[:, 3] * 0.5 + 0.5) * (W * 256.0), (PA[:, 1] / PA[:, 3] * 0.5 + 0.5) * (H * 256.0)
    Xb, Yb = (PB[:, 0] / PB[:, 3] * 0.5 + 0.5) * (W * 256.0), (PB[:, 1] / PB[:, 3] * 0.5 + 0.5) * (H * 256.0)
    dX, dY = Xb - Xa, Yb - Ya
    tt = (dX * (Py - Ya) - dY * (Px - Xa)) / -(dX * uy - dY * ux)
    a = tt - 0.5 if real else (torch.from_numpy(pr["t"]).to(f) - 0.5) + (tt - tt.detach())
    mag = sign * a
    out = color
    hz, lower = pr["horiz"], pr["O"] < pr["R"]
    for m in (hz & lower, hz & ~lower, ~hz & lower, ~hz & ~lower):               # the receiver's pair with its left, right, lower, upper neighbour
        mt = torch.from_numpy(np.nonzero(m)[0])
        out = out.index_add(0, R[mt], mag[mt, None] * (color[O[mt]] - color[R[mt]]))
    return out


def antialias_grads(dtype, color, rast, pos, tri, topo, g, boost=1.0):
    """color [H,W,C], rast [H,W,4], pos [V,4], g [H,W,C] (float32 arrays) -> dict: out [H,W,C], d_color [H,W,C], d_pos [V,4] (float64 arrays
    evaluated in ``dtype``), B and n of the dL_dpos scatter, pairs (the decisions)"""
    color, pos, g = np.asarray(color, np.float32), np.asarray(pos, np.float32).reshape(-1, 4), np.asarray(g, np.float32)
    H, W, C = color.shape
    V = len(pos)
    pr = aa_pairs(rast, pos, tri, topo)
    ct = _t(color.reshape(-1, C), dtype).requires_grad_(True)
    PA, PB = _t(pos[pr["va"]], dtype).requires_grad_(True), _t(pos[pr["vb"]], dtype).requires_grad_(True)
    out = aa_torch(ct, PA, PB, pr, W, H)
    (out * _t(g.reshape(-1, C), dtype)).sum().backward()
    d_pos = torch.zeros((V, 4), dtype=dtype)
    B, n = 0.0, 0
    if len(pr["R"]):
        ga, gb = PA.grad * boost, PB.grad * boost
        d_pos.index_add_(0, torch.from_numpy(pr["va"]), ga).index_add_(0, torch.from_numpy(pr["vb"]), gb)
        B = float(max(ga.abs().max(), gb.abs().max()))
        n = int(np.bincount(np.concatenate([pr["va"], pr["vb"]])).max())
    return dict(out=out.detach().double().numpy().reshape(H, W, C), d_color=ct.grad.double().numpy().reshape(H, W, C), d_pos=d_pos.double().numpy(), B=B, n=n, pairs=pr)


# ---- the bars of the GPU tests -------------------------------------------------------------------------------------------------------
def rel_l2(a, ref):
    d = float(np.sqrt(((np.asarray(a, np.float64) - ref) ** 2).sum()))
    n = float(np.sqrt((ref ** 2).sum()))
    return d / n if n > 0 else d


def check_bars(what, got, ref64, ref32, fp_term=0.0):
    """max |got - ref64| <= 4 max |ref32 - ref64| + fp_term; rel-L2 against ref64 <= 4x ref32's; eta = 0: equality; rows (last axis) that the
    reference leaves at zero are exactly zero.  The figures are printed before they are asserted.  -> (eta, error)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    assert np.isfinite(ref64).all() and np.isfinite(ref32).all(), what
    eta, err = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0, float(np.abs(got.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    r32, rgot = rel_l2(ref32, ref64), rel_l2(got, ref64)
    print(f"{what}: eta {eta:.3g} err {err:.3g} fixed-point term {fp_term:.3g} rel-L2 ref32 {r32:.3g} got {rgot:.3g}")
    zero_rows = ~(ref64 != 0).any(axis=-1)
    assert not got[zero_rows].any(), f"{what}: {int((got[zero_rows] != 0).any(axis=-1).sum())} rows are not zero where the reference's are"
    if eta == 0.0:
        assert np.array_equal(got, ref64.astype(np.float32)), what
    else:
        assert err <= 4.0 * eta + fp_term, (what, err, eta, fp_term)
        assert rgot <= 4.0 * r32, (what, rgot, r32)
    return eta, err
