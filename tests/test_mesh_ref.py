"""CPU: the mesh rasterizer's rule as tests/mesh_ref.py restates it -- hand-computed cases, watertightness, and the conditions on the
scenes the GPU tests (tests/test_gpu_mesh_raster.py) rasterize.  Nothing here runs the code under test."""
import numpy as np
import pytest

from tests import mesh_ref as M


def _one(px, py, W, H, zw=(0.0, 0.0, 0.0), w=(1.0, 1.0, 1.0), tri=((0, 1, 2),)):
    pos = M.clip_from_pixels(px, py, zw, w, W, H)
    return pos, M.rasterize(pos, np.array(tri, np.int32), W, H)


def test_one_triangle_at_16x16_by_hand():
    # (2, 2) (10, 2) (2, 10): the centres (i + 0.5, j + 0.5) strictly below the hypotenuse x + y = 12, i.e. i + j + 1 < 12; none lies on an edge
    _, r = _one([2, 10, 2], [2, 2, 10], 16, 16)
    j, i = np.mgrid[0:16, 0:16]
    want = (i >= 2) & (j >= 2) & (i + j + 1 < 12)
    assert np.array_equal(r["winner"] >= 0, want) and want.sum() == 28
    assert np.all(r["winner"][want] == 0) and np.all(r["second"] == -1)
    # u, v: barycentrics of vertices 0 and 1 (w = 1: affine).  At pixel (2, 2): centre (2.5, 2.5) -> v = 0.5 / 8, 1 - u - v = 0.5 / 8
    assert r["v"][2, 2] == pytest.approx(0.0625, abs=1e-12) and r["u"][2, 2] == pytest.approx(0.875, abs=1e-12)
    assert r["u"][8, 2] == pytest.approx(1 - 0.0625 - 6.5 / 8, abs=1e-12) and r["v"][2, 8] == pytest.approx(6.5 / 8, abs=1e-12)


def test_row_zero_is_clip_y_minus_one():
    pos = np.array([[-1, -1, 0, 1], [1, -1, 0, 1], [0, -0.5, 0, 1]], np.float32)           # hugs the edge y = -1
    r = M.rasterize(pos, np.array([[0, 1, 2]], np.int32), 8, 8)
    rows = np.nonzero((r["winner"] >= 0).any(axis=1))[0]
    assert rows.tolist() == [0, 1]


@pytest.mark.parametrize("size", M.HAND_SIZES)
def test_hand_scene(size):
    s, r = M.scene("hand_" + size), M.reference("hand_" + size)
    W, H = s["W"], s["H"]
    qx, qy = s["quad"]
    j, i = np.mgrid[0:H, 0:W]
    quad = (i < qx - 0.5) & (j < qy - 0.5)              # the edges through the centres of column / row 0 own them; those through column qx - 0.5 / row qy - 0.5 do not
    assert quad.any() and not quad[H - 1, W - 1] or (W, H) == (1, 1)
    win = r["winner"]
    assert np.all(np.isin(win[quad], (0, 1)))           # both windings rasterize, and the duplicates 9, 10 lose to the lower index
    assert np.all(r["second"][quad] >= 9) and np.all(r["z_second"][quad] == r["z"][quad])
    assert np.all(win[~quad] == 8)                      # behind it: the only other face that produces fragments
    assert np.all(r["z"][quad] == 0.25) and np.all(r["z"][~quad] == 0.5)
    if W > 2 and H > 2:
        assert {0, 1} <= set(win[quad].tolist())
    # the diagonal of the quad is shared: every pixel whose centre is on it went to exactly one of the two (no hole, checked above; no overlap:)
    X, Y, ok, _, _ = M.snap(s["pos"], W, H)
    t, ii, jj = M._candidates(X, Y, ok, s["tri"][:2], W, H, (0, 0, W, H))
    cov = M.covered(X, Y, s["tri"][:2], t, ii, jj)
    assert len(np.unique(jj[cov] * W + ii[cov])) == cov.sum() == quad.sum()
    # faces 2 .. 7 produce nothing: zero area, collinear, w <= 0, z/w outside [-1, 1]
    alone = M.rasterize(s["pos"], s["tri"][2:8], W, H)
    assert np.all(alone["winner"] == -1)
    assert not M.ambiguous(r, s["tri"]).any()


def test_windings_cover_the_same_pixels():
    px, py = [1.3, 13.1, 4.2], [2.2, 5.9, 14.4]
    _, a = _one(px, py, 16, 16)
    _, b = _one(px, py, 16, 16, tri=((0, 2, 1),))
    assert np.array_equal(a["winner"], b["winner"]) and (a["winner"] >= 0).sum() > 30
    assert np.allclose(a["u"], b["u"]) and not np.allclose(a["v"], b["v"])                 # vertex 1 is another vertex now


def test_depth_clip_and_nearest_wins():
    px, py = [-20, 60, -20] * 2, [-20, -20, 60] * 2
    pos = M.clip_from_pixels(px, py, [0.5, 0.5, 0.5, -0.5, -0.5, 2.5], [1, 1, 1, 1, 1, 1], 16, 16)
    r = M.rasterize(pos, np.array([[0, 1, 2], [3, 4, 5]], np.int32), 16, 16)
    z1 = r["z"].copy(); z1[r["winner"] != 1] = 0
    assert set(np.unique(r["winner"]).tolist()) == {0, 1}
    assert np.all(z1 <= 0.5) and np.all(r["z"][r["winner"] == 0] == 0.5)                   # face 1 wins where it is nearer, and is cut where z/w > 1
    assert np.all(r["second"][r["winner"] == 1] == 0)


def test_watertight_jittered_grid():
    """a jittered 24 x 16-cell grid with random w in [0.5, 4] that overhangs a 97 x 61 screen leaves no empty pixel, and no pixel twice"""
    s, r = M.scene("grid_97x61"), M.reference("grid_97x61")
    holes = int((r["winner"] < 0).sum())
    print(f"grid_97x61: {holes} holes of {r['winner'].size}")
    assert holes == 0 and r["winner"].size == 5917
    assert np.all(r["second"] == -1)                    # a single sheet: exactly one triangle per pixel


def test_snapping_margin_is_what_the_generators_promise():
    for name in M.GPU_SCENES:
        s = M.scene(name)
        dist, need = M.snap_margin(s["pos"], s["W"], s["H"])
        assert (dist > need).all(), name
    # and random vertices do land inside it: the nudge is not idle
    rng = np.random.default_rng(5)
    raw = M.clip_from_pixels(rng.uniform(0, 97, 4000), rng.uniform(0, 61, 4000), np.zeros(4000), np.ones(4000), 97, 61)
    dist, need = M.snap_margin(raw, 97, 61)
    fixed = M.unambiguous(raw, 97, 61)
    print(f"{int((dist <= need).sum())} of {dist.size} random coordinates inside the margin {need:.3g}")
    assert np.abs(fixed - raw).max() < 1e-4


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_scene_conditions(name):
    """For every scene used on the GPU: depth-ambiguous pixels (best and second-best fp64 depth within 4 eta_z) are at most 1 % of the covered
    pixels, with the reference alone; the fp32 and fp64 evaluations agree on the winner everywhere else."""
    s, r = M.scene(name), M.reference(name)
    cov = r["winner"] >= 0
    amb = M.ambiguous(r, s["tri"])
    print(f"{name}: F = {len(s['tri'])}, covered {int(cov.sum())} of {cov.size}, ambiguous {int(amb.sum())}, eta_z = {r['eta_z']:.3e}, eta_uv = {r['eta_uv']:.3e}, "
          f"fp32 and fp64 agree on {r['n_same']}")
    assert cov.any()
    assert amb.sum() <= M.AMBIGUOUS_CAP * cov.sum()
    assert r["n_same"] >= cov.sum() - amb.sum()
    assert np.all((r["u"] >= 0) & (r["v"] >= 0) & (r["u"] + r["v"] <= 1 + 1e-12))
    assert np.all((r["z"][cov] >= -1) & (r["z"][cov] <= 1))
    if name == "tiny_256":
        assert r["winner"].max() > 65535
    if name in ("grid_97x61", "coarse_200x150", "tiny_256", "fullscreen_512"):
        assert cov.all()


def test_interpolate_reference():
    rast = np.array([[0.25, 0.5, 0.1, 2.0], [0.0, 0.0, 0.0, 0.0]])
    tri = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    attr = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]])
    out, bound = M.interpolate(attr, rast, tri)
    assert np.allclose(out[0], [0.25 * 4 + 0.5 * 2 + 0.25 * 1, 10 + 10 + 2.5]) and np.all(out[1] == 0) and np.all(bound[1] == 0) and np.all(bound[0] > 0)
