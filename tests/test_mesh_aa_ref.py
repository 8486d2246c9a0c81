"""CPU: tests/mesh_aa_ref.py, the restatement the antialias kernels are held to, on cases computed by hand -- and that the scenes the GPU tests use
are not vacuous."""
import numpy as np
import pytest

from tests import mesh_aa_ref as R


def _aa(color, rast, pos, tri):
    return R.antialias(color, rast, pos, tri)


@pytest.mark.parametrize("vertical", [True, False])
def test_one_silhouette_edge_by_hand(vertical):
    """the edge at 3.75 px: pixel 3 (centre 3.5) shows the triangle, pixel 4 does not; the edge crosses at t = 0.25 of the way, a = -0.25, so P
    receives 0.25 (0 - 1): out[P] = 0.75, out[Q] = 0.  At 4.25 px pixel 4 (centre 4.5) is still outside: t = 0.75, a = +0.25, Q receives
    0.25 (1 - 0): out[Q] = 0.25, out[P] = 1."""
    for x, want_p, want_q in ((3.75, 0.75, 0.0), (4.25, 1.0, 0.25)):
        pos, tri, rast, color = R.edge_case(x, vertical)
        mask = color[..., 0] if vertical else color[..., 0].T
        assert np.all(mask[:, :4] == 1) and np.all(mask[:, 4:] == 0)
        r = _aa(color, rast, pos, tri)
        for out in (r["out64"], r["out32"].astype(np.float64)):
            o = out[..., 0] if vertical else out[..., 0].T
            assert np.all(o[:, 3] == want_p) and np.all(o[:, 4] == want_q)
            assert np.all(o[:, :3] == 1) and np.all(o[:, 5:] == 0)
        t = r["touched"] if vertical else r["touched"].T
        assert np.array_equal(np.nonzero(t.any(axis=0))[0], [3] if want_q == 0 else [4])
        assert r["eta_aa"] == 0.0 and r["n_contrib"] == 8 and (r["n_horizontal"], r["n_vertical"]) == ((8, 0) if vertical else (0, 8))


def test_a_flat_quad_never_blends_along_its_shared_edge_and_a_folded_one_does():
    rng = np.random.default_rng(5)
    color = rng.uniform(0, 1, (10, 12, 2)).astype(np.float32)
    pos, tri, rast = R.quad_case(folded=False)
    topo = R.topology(tri, 4)
    assert topo.tolist() == [[3, -1, -1], [2, -1, -1]]
    ids = rast[..., 3]
    assert ids[4, 6] == 1 and ids[5, 6] == 2                                      # the pair (6, 4) - (6, 5) straddles the shared edge
    r = _aa(color, rast, pos, tri)
    inner = np.zeros_like(r["touched"])
    inner[1:-1, 1:-1] = (ids[1:-1, 1:-1] > 0) & (ids[:-2, 1:-1] > 0) & (ids[2:, 1:-1] > 0) & (ids[1:-1, :-2] > 0) & (ids[1:-1, 2:] > 0)
    assert inner.sum() >= 10 and not r["touched"][inner].any()                    # every neighbour covered: only interior pairs, none blends
    assert r["n_not_silhouette"] >= 8 and r["n_contrib"] > 0                      # (the outer boundary does blend)
    assert np.array_equal(r["out32"][~r["touched"]], color[~r["touched"]])

    pos, tri, rast = R.quad_case(folded=True)
    ids = rast[..., 3]
    assert ids[4, 6] > 0 and ids[5, 6] == 0 and ids[5, 7] > 0                     # beyond the shared edge there is nothing now
    r = _aa(color, rast, pos, tri)
    assert r["touched"][5, 6]
    # pixel (6, 5) receives from its right neighbour (the edge crosses y = 5.5 at x = 2.25 + 3.75 * 7.5 / 6.5, t = 7.5 - x) and from the pixel
    # below (it crosses x = 6.5 at y = 1.75 + 4.25 * 6.5 / 7.5, t = y - 4.5), in that order
    a_right = (7.5 - (2.25 + 3.75 * 7.5 / 6.5)) - 0.5
    a_below = ((1.75 + 4.25 * 6.5 / 7.5) - 4.5) - 0.5
    c = color.astype(np.float64)
    want = c[5, 6] + a_right * (c[5, 7] - c[5, 6]) + a_below * (c[4, 6] - c[5, 6])
    assert np.allclose(r["out64"][5, 6], want, rtol=0, atol=1e-12)
    assert np.abs(r["out32"][5, 6] - want).max() < 4e-7


def test_topology_by_hand():
    # a fan of three triangles around the edge 0-1, a duplicated face, a face with a repeated index and one with an index out of range
    tri = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 7], [5, 6, 7], [0, 0, 1], [0, 1, 9], [2, 1, 8]], np.int32)
    topo = R.topology(tri, 9)
    assert topo[0].tolist() == [-2, 8, -1] and topo[1].tolist() == [-2, -1, -1] and topo[2].tolist() == [-2, -1, -1]
    assert topo[3].tolist() == [7, 5, 6] and topo[4].tolist() == [7, 5, 6]       # the copy is the one neighbour: its opposite vertex is one's own
    assert topo[5].tolist() == [-1, -1, -1] and topo[6].tolist() == [-1, -1, -1]
    assert topo[7].tolist() == [0, -1, -1]
    assert R.topology(np.zeros((0, 3), np.int32), 4).shape == (0, 3)


@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (1, 2)])
def test_the_smallest_images(W, H):
    """a triangle whose vertical / horizontal edge passes at 0.75 px: pixel 0 inside, pixel 1 (if there is one across it) outside"""
    pos, tri, rast, color = R.edge_case(0.75, vertical=W >= H, W=W, H=H)
    assert rast[0, 0, 3] == 1 and rast.reshape(-1, 4)[-1, 3] == (1 if W * H == 1 else 0)
    r = _aa(color, rast, pos, tri)
    assert r["out32"].shape == (H, W, 1)
    if W * H == 1:
        assert r["n_pairs"] == 0 and not r["touched"].any() and r["out32"][0, 0, 0] == 1
    else:                                                                         # t = 0.25: P receives 0.25 (0 - 1)
        assert r["out32"].reshape(-1).tolist() == [0.75, 0.0] and r["touched"].reshape(-1).tolist() == [True, False]


def test_no_faces_or_no_vertices_copy():
    color = np.random.default_rng(1).uniform(0, 1, (3, 4, 2)).astype(np.float32)
    rast = np.zeros((3, 4, 4), np.float32)
    rast[1, 1, 3] = 1.0
    for pos, tri in ((np.zeros((0, 4), np.float32), np.array([[0, 1, 2]], np.int32)), (np.ones((3, 4), np.float32), np.zeros((0, 3), np.int32))):
        r = _aa(color, rast, pos, tri)
        assert np.array_equal(r["out32"], color) and not r["touched"].any()


@pytest.mark.parametrize("name", R.GPU_SCENES)
def test_the_gpu_scenes_are_not_vacuous(name):
    covered = int((R.scene_rast(name)[..., 3] > 0).sum())
    r = R.reference(name, 3)
    touched = int(r["touched"].sum())
    print(f"{name}: {covered} covered pixels, {r['n_pairs']} pairs with two IDs, {r['n_contrib']} contributions on {touched} pixels "
          f"({100.0 * touched / max(covered, 1):.2f} %), a > 0: {r['n_pos']}, a < 0: {r['n_neg']}, horizontal {r['n_horizontal']}, vertical {r['n_vertical']}, "
          f"not a silhouette {r['n_not_silhouette']}, no exit edge {r['n_no_exit']}, eta_aa {r['eta_aa']:.3e}")
    if name in R.NON_VACUOUS:
        assert touched >= 0.01 * covered
        assert r["n_pos"] > 0 and r["n_neg"] > 0 and r["n_horizontal"] > 0 and r["n_vertical"] > 0
    if name in R.INTERIOR_SCENES:
        assert r["n_not_silhouette"] > 0
    # every pixel that receives differs from its colour in fp32 too: "the pixels that differ from color" and "the pixels that receive" are one set
    for C in R.CHANNELS:
        rc = R.reference(name, C)
        assert np.array_equal((rc["out32"] != R.colors(name, C)).any(axis=-1), rc["touched"])
        assert np.array_equal(rc["touched"], r["touched"])                        # which pixels receive does not depend on the colours


def test_every_scene_of_the_issue_has_a_silhouette_scene_beside_it():
    """the five scenes of the issue that cannot meet the bar (see tests/mesh_aa_ref.py) stay in the GPU tests; the scenes added beside them do"""
    assert set(R.AA_SCENES) - set(R.NON_VACUOUS) == {"hand_1x1", "grid_97x61", "sheets_64x48", "sphere_256", "tiny_256"}
    assert set(R.SILHOUETTE_SCENES) <= set(R.NON_VACUOUS) and len(R.SILHOUETTE_SCENES) == 4
