"""GPU: youreditableavatar_amd.mesh_shade (csrc/tgs_mesh_shade.hip) against the rules as tests/mesh_shade_ref.py restates them.

Bars, per tensor (tests/mesh_grad_ref.py ``check_bars``, unchanged; all from the restatement alone): max |got - ref64| <= 4 max |ref32 - ref64|
plus the header's fixed-point term n 2^(e-35) for the two vertex scatters (n, B of the reference's own per-pixel contributions); rel-L2 against
ref64 no larger than 4x ref32's; rows the reference leaves at zero are exactly zero.  ``rast`` is the CPU reference's, uploaded.  Pixels whose
camera-space normal lies within 1e-5 |m'| of the flip's plane may flip either way: they get a zero upstream and are left out of the forward
comparison, and at most 1 % of a scene's covered pixels may be such (asserted).  Depth takes the scenes' own clip z where it stays away from
zero (sphere_256, fullscreen_512) and 2 + z elsewhere."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_grad_ref as G
from tests import mesh_shade_ref as R

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
ALL = ("vn", "pos", "rast")
MODES = (("camera", True), ("camera", False), ("world", True), ("world", False))


def _ms():
    import youreditableavatar_amd.mesh_shade as ms
    return ms


def _dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)            # (a copy: the cached arrays are read-only)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _c2w(rot):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = rot
    return m


def _pos(z):
    p = np.zeros((len(z), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 7.0, -3.0, z, 1.0                        # (x, y and w are not read)
    return p


def run(rast, tri, vn, mode, rot, flip, z, g, need=ALL):
    """one image through ``shade`` and, with ``g``, its backward -> dict of numpy arrays: out [H,W,C], d_vn [V,3], d_pos [V,4], d_rast [H,W,4]"""
    r, v = _dev(rast, "rast" in need and g is not None), _dev(vn, "vn" in need and g is not None)
    p = None if z is None else _dev(_pos(z), "pos" in need and g is not None)
    out = _ms().shade(r[None], _dev(tri), v, normal_type=mode, c2w=_dev(_c2w(rot)) if mode == "camera" else None, flip=flip, pos_clip=p)
    assert out.shape == (1,) + rast.shape[:2] + (4 if z is None else 5,) and out.dtype == torch.float32 and out.is_cuda
    if g is None or not need:
        assert not out.requires_grad
        return dict(out=_np(out[0]))
    out.backward(_dev(g)[None])
    for t in (r, v, p):
        assert t is None or t.grad is None or (t.grad.dtype == torch.float32 and t.grad.is_cuda and t.grad.shape == t.shape)
    return dict(out=_np(out[0]), d_vn=_np(v.grad), d_pos=None if p is None else _np(p.grad), d_rast=_np(r.grad))


@functools.lru_cache(maxsize=None)
def case(name, mode, flip, depth=True):
    """the scene's inputs, its upstream (zero on the pixels that may flip either way) and the restatement in both precisions, computed once"""
    s = R.scene(name)
    rast, vn, rot = R.scene_rast(name), R.normals(name), R.rotation(name) if mode == "camera" else None
    z = R.clip_z(name) if depth else None
    g = G.upstream(name, (s["H"], s["W"], 5 if depth else 4), "shade" + mode)
    amb = np.zeros((s["H"], s["W"]), bool)
    if mode == "camera" and flip:
        amb, n_cov = R.flip_ambiguous(rast, s["tri"], vn, rot)
        assert n_cov > 0 and amb.sum() <= R.AMBIGUOUS_CAP * n_cov, (name, int(amb.sum()), n_cov)
        g[amb] = 0.0
    r64, r32 = (R.shade(f, rast, s["tri"], vn, mode, rot, flip, z, g) for f in (F64, F32))
    for a in (g, amb):
        a.setflags(write=False)
    return dict(s=s, rast=rast, vn=vn, rot=rot, z=z, g=g, amb=amb, r64=r64, r32=r32)


def check(what, c, got, need=ALL):
    r64, r32, amb = c["r64"], c["r32"], c["amb"]
    out = got["out"].copy()
    out[amb] = r64["out"][amb].astype(np.float32)                                 # left out of the forward comparison
    G.check_bars(f"{what} out ({int(amb.sum())} of {len(r64['covered'])} pixels may flip)", out, r64["out"], r32["out"])
    covered = np.zeros(amb.size, bool)
    covered[r64["covered"]] = True
    assert np.array_equal(got["out"][..., 0].reshape(-1), covered.astype(np.float32))          # the mask: exactly 1 and 0
    if "vn" in need:
        G.check_bars(f"{what} dL_dvn", got["d_vn"], r64["d_vn"], r32["d_vn"], G.fixed_point_term(r64["B_vn"], r64["n"]))
    if "pos" in need and c["z"] is not None:
        assert not got["d_pos"][:, [0, 1, 3]].any()                                # only the z column is non-zero
        G.check_bars(f"{what} dL_dz", got["d_pos"][:, 2:3], r64["d_z"][:, None], r32["d_z"][:, None], G.fixed_point_term(r64["B_z"], r64["n"]))
    if "rast" in need:
        G.check_bars(f"{what} dL_drast", got["d_rast"], r64["d_rast"], r32["d_rast"])
        assert not got["d_rast"][..., 2:].any()


def _run_case(c, mode, flip, need=ALL):
    return run(c["rast"], c["s"]["tri"], c["vn"], mode, c["rot"], flip, c["z"], c["g"], need)


# ---- against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SCENES)
def test_every_scene_in_camera_mode_with_depth(name):
    c = case(name, "camera", True)
    check(f"{name} camera flip", c, _run_case(c, "camera", True))


@pytest.mark.parametrize("name", ["grid_97x61", "sphere_256"])
@pytest.mark.parametrize("mode,flip", MODES[1:])
def test_the_other_modes_and_flip_values(name, mode, flip):
    c = case(name, mode, flip)
    check(f"{name} {mode} flip={flip}", c, _run_case(c, mode, flip))


@pytest.mark.parametrize("mode,flip", MODES)
def test_without_depth(mode, flip):
    c = case("coarse_200x150", mode, flip, depth=False)
    got = _run_case(c, mode, flip)
    assert got["out"].shape[-1] == 4 and got["d_pos"] is None
    check(f"coarse_200x150 {mode} flip={flip} C=4", c, got)


@pytest.mark.parametrize("mode,flip", MODES)
def test_each_gradient_alone_has_the_bits_it_has_together(mode, flip):
    c = case("grid_97x61", mode, flip)
    together = _run_case(c, mode, flip)
    for need in (("vn",), ("pos",), ("rast",)):
        alone = _run_case(c, mode, flip, need)
        key = {"vn": "d_vn", "pos": "d_pos", "rast": "d_rast"}[need[0]]
        assert np.array_equal(alone[key].view(np.uint32), together[key].view(np.uint32)), (mode, flip, need)
        assert all(alone[k] is None for k in ("d_vn", "d_pos", "d_rast") if k != key)
        assert np.array_equal(alone["out"].view(np.uint32), together["out"].view(np.uint32))
    plain = _run_case(c, mode, flip, ())
    assert np.array_equal(plain["out"].view(np.uint32), together["out"].view(np.uint32))
    with torch.no_grad():                                                         # no graph wanted, whatever the inputs require
        out = _ms().shade(_dev(c["rast"], True)[None], _dev(c["s"]["tri"]), _dev(c["vn"], True), normal_type=mode,
                          c2w=_dev(_c2w(c["rot"])) if mode == "camera" else None, flip=flip, pos_clip=_dev(_pos(c["z"]), True))
    assert out.grad_fn is None and np.array_equal(_np(out[0]).view(np.uint32), together["out"].view(np.uint32))


@pytest.mark.parametrize("name", ["sphere_256", "fullscreen_512"])
def test_two_runs_give_the_same_bits(name):
    c = case(name, "camera", True)
    a, b = _run_case(c, "camera", True), _run_case(c, "camera", True)
    for k in ("out", "d_vn", "d_pos", "d_rast"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("which", ["first", "last"])
def test_one_hot_upstreams(which):
    name = "grid_97x61"
    c = dict(case(name, "camera", True))
    s = c["s"]
    g = np.zeros((s["H"], s["W"], 5), np.float32)
    at = (0, 0) if which == "first" else (s["H"] - 1, s["W"] - 1)
    assert not c["amb"][at]
    g[at] = (3.0, 0.5, -1.0, 0.25, 2.0)
    c["g"] = g
    c["r64"], c["r32"] = (R.shade(f, c["rast"], s["tri"], c["vn"], "camera", c["rot"], True, c["z"], g) for f in (F64, F32))
    got = _run_case(c, "camera", True)
    check(f"{name} one-hot {which}", c, got)
    assert got["d_rast"][at][:2].any() and np.count_nonzero(got["d_rast"].reshape(-1, 4).any(axis=1)) <= 3      # the pixel, and through the depth's extremes two more


# ---- N images --------------------------------------------------------------------------------------------------------------------------
def test_three_images_with_a_matrix_each_and_shared_inputs():
    ms, name = _ms(), "grid_97x61"
    c = case(name, "camera", True)
    s, N = c["s"], 3
    rots = [R.rotation(name, f"rot{n}") for n in range(N)]
    gs = [G.upstream(name, (s["H"], s["W"], 5), f"batch{n}") for n in range(N)]
    rasts = [np.array(c["rast"]) for _ in range(N)]
    rasts[1] = rasts[1][::-1].copy()                                             # another image: the rows upside down
    tri = _dev(s["tri"])
    singles = [run(rasts[n], s["tri"], c["vn"], "camera", rots[n], True, c["z"], gs[n]) for n in range(N)]
    c2w = _dev(np.stack([_c2w(r) for r in rots]))
    for per_image in (False, True):
        rast = _dev(np.stack(rasts), True)
        vn = _dev(np.stack([c["vn"]] * N) if per_image else c["vn"], True)
        pos = _dev(np.stack([_pos(c["z"])] * N) if per_image else _pos(c["z"])[None], True)
        out = ms.shade(rast, tri, vn, c2w=c2w, pos_clip=pos)
        out.backward(_dev(np.stack(gs)))
        for n in range(N):
            assert np.array_equal(_np(out[n]).view(np.uint32), singles[n]["out"].view(np.uint32)), n
            assert np.array_equal(_np(rast.grad[n]).view(np.uint32), singles[n]["d_rast"].view(np.uint32)), n
        if per_image:
            for n in range(N):
                assert np.array_equal(_np(vn.grad[n]), singles[n]["d_vn"]) and np.array_equal(_np(pos.grad[n]), singles[n]["d_pos"]), n
        else:                                                                     # shared: the images' sum in ascending image order
            want_vn = (singles[0]["d_vn"] + singles[1]["d_vn"]) + singles[2]["d_vn"]
            want_pos = (singles[0]["d_pos"] + singles[1]["d_pos"]) + singles[2]["d_pos"]
            assert np.array_equal(_np(vn.grad).view(np.uint32), want_vn.view(np.uint32)) and vn.grad.shape == vn.shape
            assert np.array_equal(_np(pos.grad[0]).view(np.uint32), want_pos.view(np.uint32)) and pos.grad.shape == pos.shape


def test_a_singular_c2w_makes_that_image_nan_and_no_other():
    ms, name = _ms(), "hand_7x5"
    c = case(name, "camera", True)
    s = c["s"]
    bad = _c2w(c["rot"])
    bad[2, :3] = bad[1, :3]                                                       # two equal rows
    rast = _dev(np.stack([c["rast"], c["rast"]]))
    vn = _dev(c["vn"], True)
    out = ms.shade(rast, _dev(s["tri"]), vn, c2w=_dev(np.stack([_c2w(c["rot"]), bad])), pos_clip=_dev(_pos(c["z"])))
    good = run(c["rast"], s["tri"], c["vn"], "camera", c["rot"], True, c["z"], None)["out"]
    o = _np(out)
    assert np.array_equal(o[0].view(np.uint32), good.view(np.uint32))
    hit = good[..., 0] == 1.0
    assert np.isnan(o[1][hit][:, 1:4]).all() and np.array_equal(o[1][..., [0, 4]], good[..., [0, 4]]) and not o[1][~hit].any()


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def _small():
    """one triangle over 2 x 3 pixels, all covered, with generic (u, v)"""
    tri = np.array([[0, 1, 2]], np.int32)
    rast = np.zeros((2, 3, 4), np.float32)
    rast[..., 0] = [[0.125, 0.25, 0.5], [0.0625, 0.375, 0.1875]]
    rast[..., 1] = [[0.25, 0.125, 0.25], [0.5, 0.375, 0.0625]]
    rast[..., 3] = 1.0
    vn = np.array([[0.0, 0.6, 0.8], [1.0, 0.0, 0.0], [0.0, -0.8, 0.6]], np.float32)
    z = np.array([1.0, 2.0, 3.0], np.float32)
    g = G.upstream("small", (2, 3, 5), "edge")
    return tri, rast, vn, z, g


def _bars(what, tri, rast, vn, mode, rot, flip, z, g):
    got = run(rast, tri, vn, mode, rot, flip, z, g)
    r64, r32 = (R.shade(f, rast, tri, vn, mode, rot, flip, z, g) for f in (F64, F32))
    check(what, dict(r64=r64, r32=r32, amb=np.zeros(rast.shape[:2], bool), z=z), got)
    return got, r64


@pytest.mark.parametrize("mode", ["camera", "world"])
def test_a_face_with_zero_normals(mode):
    tri, rast, vn, z, g = _small()
    got = run(rast, tri, np.zeros_like(vn), mode, R.rotation("small"), True, z, g)
    assert np.array_equal(got["out"][..., 1:4], np.full((2, 3, 3), 0.5, np.float32))          # n = 0 / 1e-12 = 0, stored as exactly 0.5
    for k in ("d_vn", "d_pos", "d_rast"):
        assert np.isfinite(got[k]).all(), k
    assert np.abs(got["d_vn"]).max() > 1e9                                       # g_n / 1e-12: F.normalize's clamp passes the gradient on


def test_exactly_one_covered_pixel():
    tri, rast, vn, z, g = _small()
    one = np.zeros_like(rast)
    one[1, 1] = rast[1, 1]
    got, r64 = _bars("one covered pixel", tri, one, vn, "camera", R.rotation("small"), True, z, g)
    assert got["out"][1, 1, 4] == 0.0 and got["out"][1, 1, 0] == 1.0 and not r64["d_z"].any() and not got["d_pos"].any()     # dmin = dmax


def test_a_constant_z_ties_every_pixel():
    tri, rast, vn, _, g = _small()
    z = np.ones(3, np.float32)
    got, r64 = _bars("constant z", tri, rast, vn, "world", None, True, z, g)
    assert not r64["out"][..., 4].any() and not got["out"][..., 4].any()         # every d is dmin: the restatement ties exactly, and so does the kernel
    assert np.abs(r64["d_rast"]).max() > 0.0


@pytest.mark.parametrize("what", ["no covered pixel", "F = 0", "V = 0", "no pixels"])
def test_empty_inputs(what):
    ms = _ms()
    tri, rast, vn, z, g = _small()
    if what == "no covered pixel":
        rast = np.zeros_like(rast)
    if what == "F = 0":
        tri = np.zeros((0, 3), np.int32)
    if what == "V = 0":
        vn, z = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
    if what == "no pixels":
        rast, g = np.zeros((0, 3, 4), np.float32), np.zeros((0, 3, 5), np.float32)
    for mode in ("camera", "world"):
        got = run(rast, tri, vn, mode, R.rotation("small"), True, z, g)
        assert got["out"].shape == rast.shape[:2] + (5,) and not got["out"].any()           # an all-zero depth channel, and no error
        assert got["d_vn"].shape == vn.shape and not got["d_vn"].any() and not got["d_pos"].any() and not got["d_rast"].any()
    assert ms.shade(_dev(rast)[None], _dev(tri), _dev(vn), normal_type="world").shape == (1,) + rast.shape[:2] + (4,)


def test_a_nan_upstream():
    tri, rast, vn, z, g = _small()
    g = g.copy()
    g[1, 2, 2] = np.nan                                                           # in a normal channel of one pixel
    got = run(rast, tri, vn, "camera", R.rotation("small"), True, z, g)
    assert np.isnan(got["d_vn"]).all()                                            # loud, not partial
    assert np.isfinite(got["d_pos"]).all() and got["d_pos"][:, 2].any()           # the depth's gradient does not pass through it
    nan_rows = np.isnan(got["d_rast"][..., :2]).any(axis=-1)
    assert nan_rows[1, 2] and nan_rows.sum() == 1 and not got["d_rast"][..., 2:].any()


# ---- render ----------------------------------------------------------------------------------------------------------------------------
def _render_inputs():
    from youreditableavatar_amd import scenes
    s = R.scene("sphere_256")
    cam = scenes.orbit_camera(256, 256, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    mvp = np.ascontiguousarray(np.asarray(cam.projmatrix, np.float32).T)[None]   # pos_clip = [verts, 1] @ mvp^T
    verts = np.asarray(s["verts"], np.float32) + np.float32(0.01) * R.normals("grid_97x61")[:1]       # (off the origin by a hair)
    return verts, s["tri"], mvp, _c2w(R.rotation("sphere_256"))[None]


def test_render_antialiases_the_packed_map_as_three_calls_would():
    import youreditableavatar_amd.mesh_raster_grad as dr
    ms = _ms()
    verts, tri, mvp, c2w = _render_inputs()
    v, t = _dev(verts), _dev(tri)
    out = ms.render(dr.RasterizeCudaContext(), v, t, _dev(mvp), (256, 256), c2w=_dev(c2w))
    assert set(out) == {"opacity", "comp_normal", "comp_depth", "mask", "rast", "pos_clip"}
    assert out["opacity"].shape == (1, 256, 256, 1) and out["comp_normal"].shape == (1, 256, 256, 3) and out["comp_depth"].shape == (1, 256, 256, 1)
    assert out["mask"].dtype == torch.bool and torch.equal(out["mask"], out["rast"][..., 3:] > 0) and 30000 < int(out["mask"].sum()) < 45000
    from youreditableavatar_amd import mesh_geom
    packed = ms.shade(out["rast"], t, mesh_geom.vertex_normals(v, t), c2w=_dev(c2w), pos_clip=out["pos_clip"])
    for key, lo, hi in (("opacity", 0, 1), ("comp_normal", 1, 4), ("comp_depth", 4, 5)):
        want = dr.antialias(packed[..., lo:hi].contiguous(), out["rast"], out["pos_clip"], t)
        assert torch.equal(out[key].contiguous().view(torch.int32), want.view(torch.int32)), key
    assert not torch.equal(out["opacity"], packed[..., 0:1])                      # (the silhouette was blended)
    no_depth = ms.render(None, v, t, _dev(mvp), (256, 256), normal_type="world", depth=False)
    assert "comp_depth" not in no_depth and no_depth["comp_normal"].shape == (1, 256, 256, 3)


def test_render_does_not_wait_for_the_device():
    """forward and backward under the framework's synchronisation check: with the normals' topology and the antialias topology given, nothing
    in ``render`` reads back; ``validate=True`` does (the detector is seen to work), and so does building the incidence per call"""
    import youreditableavatar_amd.mesh_raster_grad as dr
    from youreditableavatar_amd import mesh_geom
    ms = _ms()
    verts, tri, mvp, c2w = _render_inputs()
    t, m, c = _dev(tri), _dev(mvp), _dev(c2w)
    topo, inc = dr.antialias_construct_topology_hash(t), mesh_geom.mesh_topology(t, len(verts), edges=False)
    v = _dev(verts, True)
    up = _dev(G.upstream("sphere_256", (1, 256, 256, 3), "sync"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in (dict(c2w=c), dict(normal_type="world", depth=False), dict(c2w=c, flip=False, depth=False)):
            out = ms.render(None, v, t, m, (256, 256), topology_hash=topo, normals_topology=inc, **kw)
            (out["comp_normal"] * up).sum().backward()
        with pytest.raises(RuntimeError, match="synchroniz"):
            ms.render(None, v, t, m, (256, 256), c2w=c, topology_hash=topo, normals_topology=inc, validate=True)
        with pytest.raises(RuntimeError, match="synchroniz"):
            ms.render(None, v, t, m, (256, 256), c2w=c, topology_hash=topo)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(v.grad).all() and bool(v.grad.abs().sum() > 0)


def _unfused(verts, tri, mvp, c2w, up, dtype):
    """the same chain out of mesh_raster_grad and the framework calls of the renderer's lines, those calls evaluated in ``dtype``"""
    import youreditableavatar_amd.mesh_raster_grad as dr
    from youreditableavatar_amd import mesh_geom
    H = W = 256
    pos = torch.matmul(torch.nn.functional.pad(verts, (0, 1), value=1.0), mvp.permute(0, 2, 1)).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, (H, W))
    mask = rast[..., 3:] > 0
    opacity = dr.antialias(mask.float(), rast, pos, tri)
    vn = mesh_geom.vertex_normals(verts, tri)
    gb, _ = dr.interpolate(vn, rast, tri)
    gb = torch.matmul(torch.linalg.inv(c2w[:, :3, :3].to(dtype)), gb.to(dtype).view(-1, H * W, 3)[0][:, :, None])
    gb = torch.where(gb[:, 2:3] < 0, -gb, gb).view(-1, H, W, 3)
    gb = torch.nn.functional.normalize(gb, dim=-1)
    normal = torch.lerp(torch.zeros_like(gb), (gb + 1.0) / 2.0, mask.to(dtype)).float()
    normal = dr.antialias(normal, rast, pos, tri)
    gd, _ = dr.interpolate(pos[0, :, :3].contiguous(), rast, tri)
    gd = 1.0 / (gd[..., 2:3].to(dtype) + 1e-7)
    hi, lo = torch.max(gd[mask[..., 0]]), torch.min(gd[mask[..., 0]])
    depth = torch.lerp(torch.zeros_like(gd), (gd - lo) / (hi - lo + 1e-7), mask.to(dtype)).float()
    depth = dr.antialias(depth, rast, pos, tri)
    return (opacity * up[..., 0:1]).sum() + (normal * up[..., 1:4]).sum() + (depth * up[..., 4:5]).sum(), rast


def test_render_gradient_to_the_vertices_through_the_whole_chain():
    """dL_dverts of a seeded loss: render against the unfused chain.  ref64 is the chain with its framework calls in float64, ref32 the chain as the
    renderer runs it (float32); the native calls are the same in both, so eta is the framework calls' float32 noise alone."""
    import youreditableavatar_amd.mesh_raster_grad as dr
    from youreditableavatar_amd import mesh_geom
    ms = _ms()
    verts, tri, mvp, c2w = _render_inputs()
    t, m, c = _dev(tri), _dev(mvp), _dev(c2w)
    with torch.no_grad():
        first = ms.render(None, _dev(verts), t, m, (256, 256), c2w=c)
    amb, n_cov = R.flip_ambiguous(_np(first["rast"][0]), tri, _np(mesh_geom.vertex_normals(_dev(verts), t)), c2w[0, :3, :3])
    assert n_cov > 30000 and amb.sum() <= R.AMBIGUOUS_CAP * n_cov, (int(amb.sum()), n_cov)
    wide = amb.copy()                                                             # antialias blends a pixel into its four neighbours: they get a zero upstream too
    wide[1:] |= amb[:-1]; wide[:-1] |= amb[1:]; wide[:, 1:] |= amb[:, :-1]; wide[:, :-1] |= amb[:, 1:]
    up = G.upstream("sphere_256", (256, 256, 5), "render", smooth=True)
    up[wide, 1:4] = 0.0
    up = up[None]
    refs = []
    for dtype in (F64, F32):
        v = _dev(verts, True)
        loss, rast = _unfused(v, t, m, c, _dev(up), dtype)
        loss.backward()
        refs.append(_np(v.grad).astype(np.float64))
    assert torch.equal(rast, first["rast"])
    v = _dev(verts, True)
    out = ms.render(dr.RasterizeCudaContext(), v, t, m, (256, 256), c2w=c)
    u = _dev(up)
    ((out["opacity"] * u[..., 0:1]).sum() + (out["comp_normal"] * u[..., 1:4]).sum() + (out["comp_depth"] * u[..., 4:5]).sum()).backward()
    G.check_bars("sphere_256 render dL_dverts", _np(v.grad), refs[0], refs[1])
