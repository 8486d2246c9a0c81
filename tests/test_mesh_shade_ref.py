"""CPU: the restatement of the mesh shading rules (tests/mesh_shade_ref.py) checks itself: its autograd against central finite differences in
float64, the depth's tie rule against the header's formulas written out by hand, and its numbers against the chain of framework calls it
replaces (interpolate -> matmul -> where -> normalize -> lerp) written out in torch."""
import numpy as np
import pytest
import torch

from tests import mesh_grad_ref as G
from tests import mesh_shade_ref as R

F64 = torch.float64
FD_SCENES = ("hand_7x5", "grid_97x61")
FD_STEP = 2.0 ** -10
FD_MARGIN = 6.0 * FD_STEP          # pixels with |m'.z| below it get a zero upstream: a step moves m' by up to (|du| + |dv|) max |a_i - a_2| <= 4 steps, and may cross the flip


def _case(name, mode, flip, depth, tag="fd"):
    s = R.scene(name)
    rast, vn = R.scene_rast(name), R.normals(name)
    rot = R.rotation(name) if mode == "camera" else None
    zattr = R.clip_z(name) if depth else None
    g = G.upstream(name, (s["H"], s["W"], 5 if depth else 4), tag + mode)
    if mode == "camera" and flip:
        pix, vid, VN3, uv, _ = R._gather(F64, rast, s["tri"], vn, None)
        with torch.no_grad():
            m = R.transformed(VN3, uv, "camera", G._t(rot, F64), False)
        near = np.zeros(s["H"] * s["W"], bool)
        near[pix] = (m[:, 2].abs() <= FD_MARGIN).numpy()
        assert near.sum() <= 0.05 * max(len(pix), 1)
        g[near.reshape(s["H"], s["W"])] = 0.0
    return s, rast, vn, rot, zattr, g


def _loss(s, rast, vn, rot, zattr, g, mode, flip):
    return float((R.shade(F64, rast, s["tri"], vn, mode, rot, flip, zattr)["out"] * g.astype(np.float64)).sum())


@pytest.mark.parametrize("name", FD_SCENES)
@pytest.mark.parametrize("mode", ["camera", "world"])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("depth", [False, True])
def test_autograd_agrees_with_central_differences(name, mode, flip, depth):
    """directional derivatives along seeded directions of vn, of the z column and of rast's u, v.  The inputs are float32 arrays, so a step is a
    float32 step: 2^-10 of a unit-sized input, exactly representable next to it for most entries; the difference quotient uses the steps taken."""
    s, rast, vn, rot, zattr, g = _case(name, mode, flip, depth)
    ref = R.shade(F64, rast, s["tri"], vn, mode, rot, flip, zattr, g)
    rng = np.random.default_rng(5)
    h = FD_STEP

    def check(what, grad, base, run):
        for _ in range(3):
            direction = rng.uniform(-1.0, 1.0, base.shape)
            up, down = (base.astype(np.float64) + h * direction).astype(np.float32), (base.astype(np.float64) - h * direction).astype(np.float32)
            taken = up.astype(np.float64) - down.astype(np.float64)
            want = float((grad * taken).sum())
            got = run(up) - run(down)
            scale = float(np.abs(grad * taken).sum()) + 1e-30
            print(f"{name} {mode} flip={flip} depth={depth} {what}: autograd {want:.9g} differences {got:.9g}")
            assert abs(got - want) <= 2e-4 * scale, (what, got, want, scale)     # the step's second-order term: h^2 against h
    check("vn", ref["d_vn"], vn, lambda x: _loss(s, rast, x, rot, zattr, g, mode, flip))
    if depth:
        check("z", ref["d_z"], zattr, lambda x: _loss(s, rast, vn, rot, x, g, mode, flip))

    def with_uv(x):
        r = np.array(rast)
        r[..., :2] = x
        return r
    check("rast", ref["d_rast"][..., :2], np.array(rast[..., :2]), lambda x: _loss(s, with_uv(x), vn, rot, zattr, g, mode, flip))
    assert not ref["d_rast"][..., 2:].any()


def _tie_case():
    """one triangle, 2 x 2 pixels: pixels 0 and 1 share (u, v) and tie for dmax, pixel 2 holds dmin alone, pixel 3 is empty"""
    tri = np.array([[0, 1, 2]], np.int32)
    rast = np.zeros((2, 2, 4), np.float32)
    rast[0, 0] = rast[0, 1] = (0.25, 0.25, 0.0, 1.0)
    rast[1, 0] = (0.125, 0.125, 0.0, 1.0)
    vn = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
    zattr = np.array([1.0, 2.0, 3.0], np.float32)
    g = np.zeros((2, 2, 5), np.float32)
    g[..., 4] = [[0.75, -0.5], [0.25, 9.0]]
    return tri, rast, vn, zattr, g


def test_depth_ties_share_evenly_as_the_header_says():
    tri, rast, vn, zattr, g = _tie_case()
    ref = R.shade(F64, rast, tri, vn, "world", None, True, zattr, g)
    uv = rast.reshape(-1, 4)[:3, :2].astype(np.float64)
    w = np.stack([uv[:, 0], uv[:, 1], 1.0 - uv[:, 0] - uv[:, 1]], 1)
    z = w @ zattr.astype(np.float64)
    d = 1.0 / (z + 1e-7)
    assert d[0] == d[1] > d[2]
    dmin, dmax = d.min(), d.max()
    r = dmax - dmin + 1e-7
    assert np.allclose(ref["out"].reshape(-1, 5)[:3, 4], (d - dmin) / r, rtol=0, atol=1e-15) and not ref["out"][1, 1].any()
    gp = g.reshape(-1, 5)[:3, 4].astype(np.float64)
    S1, S2 = gp.sum(), (gp * (d - dmin)).sum()
    gd = gp / r
    gd[:2] += (-S2 / r ** 2) / 2.0                                               # two pixels attain dmax
    gd[2] += -S1 / r + S2 / r ** 2                                               # one attains dmin
    gz = -gd * d * d
    want_z = (w * gz[:, None]).sum(0)
    tol = 1e-13 * (np.abs(gp).sum() / r + abs(S2) / r ** 2) * float((d * d).max()) * 3.0       # the terms cancel: rounding is relative to them, not to the sum
    assert np.abs(want_z).max() > 1e3 * tol
    assert np.allclose(ref["d_z"], want_z, rtol=0, atol=tol), (ref["d_z"], want_z, tol)
    want_rast = np.stack([gz * (zattr[0] - zattr[2]), gz * (zattr[1] - zattr[2])], 1)
    assert np.allclose(ref["d_rast"].reshape(-1, 4)[:3, :2], want_rast, rtol=0, atol=2.0 * tol)
    assert not ref["d_rast"].reshape(-1, 4)[3].any() and not ref["d_vn"].any()  # the normal's channels had a zero upstream


def test_one_covered_pixel_and_none():
    tri, rast, vn, zattr, g = _tie_case()
    one = np.zeros_like(rast)
    one[1, 0] = rast[1, 0]
    ref = R.shade(F64, one, tri, vn, "world", None, True, zattr, g)
    assert ref["out"][1, 0, 4] == 0.0 and ref["out"][1, 0, 0] == 1.0 and not ref["d_z"].any()   # dmin = dmax: d - dmin = 0, and its gradient cancels
    none = R.shade(F64, np.zeros_like(rast), tri, vn, "world", None, True, zattr, g)
    assert not none["out"].any() and not none["d_vn"].any() and not none["d_z"].any() and not none["d_rast"].any()


def _chain(dtype, rast, tri, vn, mode, rot, flip, zattr):
    """the framework calls the renderer makes, in its order, on whole images -> (normal map [1,H,W,3], depth map [1,H,W,1] or None, the leaves)"""
    rast = np.asarray(rast, np.float32)
    H, W = rast.shape[:2]
    pix, vid = G.covered(rast, tri, len(vn))
    vn_t = G._t(vn, dtype).requires_grad_(True)
    uv = G._t(rast.reshape(-1, 4)[pix][:, :2], dtype)
    rows = torch.from_numpy(pix)

    def interpolate(attr):                                                        # [V,C] -> [1,H,W,C], zeros where nothing is hit
        C = attr.shape[1]
        vals = G.interpolate_torch(attr[torch.from_numpy(vid.reshape(-1))].reshape(-1, 3, C), uv)
        return torch.zeros((H * W, C), dtype=dtype).index_put((rows,), vals).reshape(1, H, W, C)
    mask = torch.from_numpy((rast[..., 3:] > 0).reshape(1, H, W, 1))
    gb = interpolate(vn_t)
    if mode == "world":
        gb = torch.nn.functional.normalize(gb, dim=-1)
        gb = torch.cat([gb[..., 1:2], gb[..., 2:3], gb[..., 0:1]], -1)
    else:
        c2w = torch.eye(4, dtype=dtype)[None].clone()
        c2w[0, :3, :3] = G._t(rot, dtype)
        gb = torch.matmul(torch.linalg.inv(c2w[:, :3, :3]), gb.view(-1, H * W, 3)[0][:, :, None])
        if flip:
            gb = torch.where(gb[:, 2:3] < 0, -gb, gb)
        gb = torch.nn.functional.normalize(gb.view(-1, H, W, 3), dim=-1)
    normal = torch.lerp(torch.zeros_like(gb), (gb + 1.0) / 2.0, mask.to(dtype))
    depth, z_t = None, None
    if zattr is not None:
        z_t = G._t(zattr, dtype).requires_grad_(True)
        gd = 1.0 / (interpolate(z_t[:, None]) + 1e-7)
        hi, lo = torch.max(gd[mask[..., 0]]), torch.min(gd[mask[..., 0]])
        depth = torch.lerp(torch.zeros_like(gd), (gd - lo) / (hi - lo + 1e-7), mask.to(dtype))
    return normal, depth, vn_t, z_t


@pytest.mark.parametrize("name", FD_SCENES)
@pytest.mark.parametrize("mode,flip", [("camera", True), ("camera", False), ("world", True)])
def test_the_written_out_chain_gives_the_same_numbers(name, mode, flip):
    s, rast, vn, rot, zattr, g = _case(name, mode, flip, True, tag="chain")
    ref = R.shade(F64, rast, s["tri"], vn, mode, rot, flip, zattr, g)
    normal, depth, vn_t, z_t = _chain(F64, rast, s["tri"], vn, mode, rot, flip, zattr)
    assert np.allclose(normal[0].detach().numpy(), ref["out"][..., 1:4], rtol=0, atol=1e-13)
    assert np.allclose(depth[0].detach().numpy(), ref["out"][..., 4:5], rtol=0, atol=1e-12)
    g_t = torch.from_numpy(g.astype(np.float64))
    ((normal[0] * g_t[..., 1:4]).sum() + (depth[0] * g_t[..., 4:5]).sum()).backward()
    for what, got, want in (("d_vn", vn_t.grad.numpy(), ref["d_vn"]), ("d_z", z_t.grad.numpy(), ref["d_z"])):
        err, size = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"{name} {mode} flip={flip} {what}: chain against restatement {err:.3g} of {size:.3g}")
        assert err <= 1e-10 * size, (what, err, size)


def test_the_inverse_and_the_flip_margin():
    rot = R.rotation("grid_97x61")
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6) and np.linalg.det(rot.astype(np.float64)) > 0
    inv = R.inverse3(G._t(rot, F64)).numpy()
    assert np.allclose(inv, np.linalg.inv(rot.astype(np.float64)), rtol=0, atol=1e-14)
    for name in ("hand_7x5", "grid_97x61"):                                       # (the GPU suite asserts the cap on every scene it runs)
        amb, n = R.flip_ambiguous(R.scene_rast(name), R.scene(name)["tri"], R.normals(name), R.rotation(name))
        assert n > 0 and amb.sum() <= R.AMBIGUOUS_CAP * n
