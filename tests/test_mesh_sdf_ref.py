"""CPU: the float64 restatement of the mesh signed distance (tests/mesh_sdf_ref.py) against closed forms: the unit cube with points whose rays pass
exactly through edges and corners, the regular tetrahedron and octahedron in their face, edge and vertex regions, the cube without its lid, two
overlapping cubes, and a zero-area face that changes nothing."""
import itertools

import numpy as np
import pytest

from tests import mesh_sdf_ref as R

DYADIC = (-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5)


def box_sdf(p, lo=0.0, hi=1.0):
    """the signed distance to the solid box [lo, hi]^3, positive inside, in float64"""
    q = np.abs(np.asarray(p, np.float64) - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return -(np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0))


def shuffled(v, f, seed):
    """the same surface with the vertices renumbered and every face rolled or turned over: parity and distance must not notice"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))
    inv = np.argsort(perm)
    f2 = inv[f]
    for k in range(len(f2)):
        f2[k] = np.roll(f2[k], rng.integers(3))
        if rng.integers(2):
            f2[k] = f2[k][::-1]
    return v[perm], f2.astype(np.int32)


@pytest.mark.parametrize("seed", [None, 1, 2, 3])
def test_unit_cube_with_rays_through_edges_and_corners(seed):
    v, f = R.cube(0.0, 1.0)
    if seed is not None:
        v, f = shuffled(v, f, seed)
    pts = np.array(list(itertools.product(DYADIC, repeat=3)), np.float32)
    out = R.query(v, f, pts)
    want = box_sdf(pts)
    assert np.abs(out["dist"] - np.abs(want)).max() <= 1e-15
    # the tie rule is a shift of the point by (+eps, +eps^2) in the ray's plane: on the cube a ray along k counts one face exactly when the
    # other two coordinates are in [0, 1) and p_k is in [0, 1) (the face at 1 is above, the face at 0 is not)
    half_open = (pts >= 0.0) & (pts < 1.0)
    for k in range(3):
        assert np.array_equal(out["parity"][:, k], half_open.all(axis=1)), k
    on = want == 0.0
    assert on.sum() == 98 and np.array_equal(out["inside"], half_open.all(axis=1) | on)
    assert np.array_equal(out["sdf"], np.where(on, 0.0, np.where(out["inside"], np.abs(want), -np.abs(want))).astype(np.float32))
    assert not np.signbit(out["sdf"][on]).any()                                  # d == 0: +0.0
    assert not out["flag"].any()                                                # exact zeros are ties, not margins; the points on the cube carry no flag
    tri = v[f[out["face"]]].astype(np.float64)
    assert np.abs(R.point_triangle_distance(pts, tri[:, 0], tri[:, 1], tri[:, 2]) - out["dist"]).max() == 0.0
    assert np.abs(np.linalg.norm(pts - out["closest"].astype(np.float64), axis=1) - out["dist"]).max() <= 1e-7


def test_unit_cube_axis_aligned_points_and_lowest_face():
    v, f = R.cube(0.0, 1.0)
    pts = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 1.5], [0.5, -2.0, 0.5], [1.5, 1.5, 0.5], [2.0, 2.0, 2.0], [0.25, 0.5, 0.5], [0.5, 0.5, 0.9375]], np.float32)
    out = R.query(v, f, pts)
    assert np.array_equal(out["sdf"], np.array([0.5, -0.5, -2.0, -np.sqrt(0.5), -np.sqrt(3.0), 0.25, 0.0625], np.float32))
    assert np.array_equal(out["inside"], [True, False, False, False, False, True, True])
    assert out["face"][0] == 0                                                  # the centre is at 0.5 from all twelve faces: the lowest
    d = R.point_triangle_distance(pts[0], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert np.all(d == 0.5)
    assert np.array_equal(out["closest"][4], [1.0, 1.0, 1.0]) and np.array_equal(out["closest"][3], [1.0, 1.0, 0.5])
    bad = R.query(v, f, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, 0.5]], np.float32))
    assert np.isnan(bad["sdf"][:2]).all() and np.array_equal(bad["face"][:2], [-1, -1]) and not bad["inside"][:2].any() and bad["sdf"][2] == 0.5


def test_tetrahedron_and_octahedron_regions():
    s3 = np.sqrt(3.0)
    v, f = R.tetrahedron()
    pts = np.array([[3, 3, 3], [-2, -2, -2], [2.5, 0, 0], [0, 0, 0], [0.25, 0.125, -0.0625]], np.float32)
    out = R.query(v, f, pts)
    want = np.array([2.0 * s3, (2.0 - 1.0 / 3.0) * s3, 1.5, 1.0 / s3])            # the vertex (1, 1, 1), the face opposite it, the edge through (1, 0, 0), the centre
    assert np.abs(out["dist"][:4] - want).max() <= 1e-14
    assert np.array_equal(out["inside"], [False, False, False, True, True])
    assert np.array_equal(out["closest"][0], [1, 1, 1]) and np.array_equal(out["closest"][2], [1, 0, 0])
    assert np.abs(out["closest"][1].astype(np.float64) + 1.0 / 3.0).max() <= 1e-7
    planes = np.array([[1, 1, -1], [1, -1, 1], [-1, 1, 1], [-1, -1, -1]], np.float64)    # n . x <= 1 inside
    assert abs(out["dist"][4] - (1.0 - (planes @ pts[4].astype(np.float64)).max()) / s3) <= 1e-15
    assert np.array_equal(out["sdf"], np.where(out["inside"], 1, -1) * out["dist"].astype(np.float32))

    v, f = R.octahedron()
    pts = np.array([[2, 0, 0], [1, 1, 1], [1, 1, 0], [0, 0, 0], [0, 0, -3], [-1, -1, 0.5]], np.float32)
    out = R.query(v, f, pts)
    #                 vertex  face        edge          centre      vertex  face -x - y + z = 1 at distance (2.5 - 1) / sqrt 3
    want = np.array([1.0, 2.0 / s3, np.sqrt(0.5), 1.0 / s3, 2.0, 1.5 / s3])
    assert np.abs(out["dist"] - want).max() <= 1e-14
    assert np.array_equal(out["inside"], [False, False, False, True, False, False])
    assert np.array_equal(out["closest"][0], [1, 0, 0]) and np.array_equal(out["closest"][2], [0.5, 0.5, 0]) and np.array_equal(out["closest"][4], [0, 0, -1])
    assert np.abs(out["closest"][1].astype(np.float64) - 1.0 / 3.0).max() <= 1e-7
    assert out["parity"][3].all() and not out["parity"][[0, 1, 2, 4, 5]].any()   # through the apexes and the equator: every ray counted once or not at all
    assert out["face"][3] == 0 and out["face"][0] == 0                         # eight faces and four faces tie: the lowest


def test_cube_without_its_lid_is_inside_by_majority():
    v, f = R.cube(0.0, 1.0, lid=False)
    assert len(f) == 10
    pts = np.array([[0.3, 0.6, 0.4], [0.5, 0.5, 0.5], [0.3, 0.6, 1.5], [0.3, 0.6, -0.5], [1.5, 0.6, 0.4]], np.float32)
    out = R.query(v, f, pts)
    assert np.array_equal(out["parity"][0], [True, True, False]) and np.array_equal(out["parity"][1], [True, True, False])     # the ray along z leaves through the opening
    assert np.array_equal(out["inside"], [True, True, False, False, False])
    assert not out["parity"][2].any() and not out["parity"][4].any() and np.array_equal(out["parity"][3], [False, False, True])   # one odd ray of three: outside
    assert out["sdf"][0] == np.float32(0.3) and out["sdf"][1] == 0.5


def test_overlapping_cubes_make_the_overlap_outside():
    v, f = R.two_cubes()
    pts = np.array([[-0.3, -0.3, -0.3], [0.3, 0.1, 0.0], [0.8, 0.5, 0.4], [2.0, 2.0, 2.0]], np.float32)
    out = R.query(v, f, pts)
    assert np.array_equal(out["inside"], [True, False, True, False])            # in the first only, in both, in the second only, in neither
    assert not out["parity"][1].any()
    assert abs(out["dist"][1] - 0.2) <= 1e-7                                    # the first cube's face at x = 0.5, inside the second cube


def test_a_zero_area_face_changes_nothing():
    v, f = R.cube(0.0, 1.0)
    v2 = np.concatenate([v, np.array([[0.5, 0.0, 0.0]], np.float32)])
    f2 = np.concatenate([f, np.array([[0, 8, 1], [0, 0, 1], [3, 3, 3]], np.int32)])   # on the cube's edge: three points on a line; a vertex named twice; a single point
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-0.5, 1.5, (300, 3)), np.array(list(itertools.product(DYADIC[:6], repeat=3)))]).astype(np.float32)
    a, b = R.query(v, f, pts), R.query(v2, f2, pts)
    for k in ("sdf", "dist", "face", "closest", "inside", "parity"):
        assert np.array_equal(a[k], b[k]), k
    alone = R.query(v2, np.array([[0, 8, 1]], np.int32), np.array([[0.25, 1.0, 0.0], [2.0, 0.0, 0.0], [0.5, 0.0, 0.0]], np.float32))   # as its three segments
    assert np.array_equal(alone["sdf"], np.array([-1.0, -1.0, 0.0], np.float32)) and np.array_equal(alone["inside"], [False, False, True])


def test_icosphere_and_ulp():
    v, f = R.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3) and np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()           # closed
    rng = np.random.default_rng(6)
    pts = rng.uniform(-1.2, 1.2, (400, 3)).astype(np.float32)
    out = R.query(v, f, pts)
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    clear = np.abs(r - 1.0) > 0.03                                               # the faces lie within 0.02 below the sphere
    assert np.array_equal(out["inside"][clear], (r < 1.0)[clear]) and np.abs(out["dist"] - np.abs(1.0 - r)).max() < 0.03
    assert (out["parity"].all(axis=1) | ~out["parity"].any(axis=1)).all() and not out["flag"].any()
    dent = R.icosphere(2, dent=0.3)[0]
    assert np.linalg.norm(dent[np.argmax(v[:, 2])]) < 0.71 and np.array_equal(dent[v[:, 2] < 0.6], v[v[:, 2] < 0.6])
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.75) == 2.0 ** -24 and R.ulp32(0.0) == 2.0 ** -149
