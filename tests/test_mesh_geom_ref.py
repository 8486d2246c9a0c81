"""CPU: tests/mesh_geom_ref.py, the torch restatement of the mesh-geometry rules, against what the reference's own functions returned
(tests/golden/ref_mesh_geom_fixture.npz) and against central finite differences; and the conditions the GPU comparisons rest on, so that none of
them is a coin toss: how far every vertex's normal sum is from the 1e-20 threshold, and how much of it cancels."""
import numpy as np
import pytest
import torch

from tests import mesh_geom_ref as R

ROUND_OFF = 1e-12                       # float64 against float64: the orders of the sums differ


def test_the_restatement_equals_the_fixture():
    fx = R.fixture()
    for name in R.FIXTURE_SCENES:
        m = R.scene(name)
        assert np.array_equal(fx[f"{name}.v_pos"], m["v_pos"], equal_nan=True) and np.array_equal(fx[f"{name}.faces"], m["faces"]) and len(m["faces"]) != 3
        assert fx[f"{name}.v_pos"].dtype == np.float32 and np.array_equal(fx[f"{name}.g_normals"], R.upstream(name, "random"))
        edges = R.edges_of(torch.tensor(m["faces"])).numpy()
        assert edges.dtype == np.int64 and np.array_equal(edges, fx[f"{name}.edges"])                # integers exact
        for what, key in (("normals", "compute_normal"), ("normals", "v_nrm"), ("consistency_of_normals", "normal_consistency"), ("laplacian", "laplacian")):
            (v64, g64), _ = R.reference(name, what)
            want = fx[f"{name}.{key}"]
            assert np.array_equal(np.isfinite(want), np.isfinite(v64)), (name, key)
            assert np.allclose(v64, want, rtol=0, atol=ROUND_OFF, equal_nan=True), (name, key)
            if key == "v_nrm":
                continue
            wg = fx[f"{name}.{key}.grad"]
            fin = np.isfinite(wg).all(axis=1)
            assert np.array_equal(fin, np.isfinite(g64).all(axis=1)), (name, key)                    # which rows are non-finite, row-wise
            assert np.allclose(g64[fin], wg[fin], rtol=0, atol=ROUND_OFF * max(1.0, np.abs(wg[fin]).max())), (name, key)
    assert (~np.isfinite(fx["fan.compute_normal.grad"]).all(axis=1)).sum() > 0 and np.isfinite(fx["fan.compute_normal"]).all()
    assert (fx["traps.edges"][:, 0] == fx["traps.edges"][:, 1]).sum() == 4                           # the pairs (i, i) are kept


def test_the_cosine_is_the_installed_torchs():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 3, dtype=torch.float64, generator=g) * torch.logspace(-10, 0, 64, dtype=torch.float64)[:, None]
    y = torch.randn(64, 3, dtype=torch.float64, generator=g) * 1e-8
    x[0] = 0.0
    for a, b in ((x, y), (x, x), (y, y)):
        assert torch.equal(R.cosine(a, b), torch.cosine_similarity(a, b, dim=-1))
    e = torch.zeros((0, 2), dtype=torch.int64)
    assert torch.isnan(R.normal_consistency(x, e))                                                   # the mean of nothing


def test_a_pair_of_equal_indices_adds_nothing_to_the_laplacian():
    v, f = R.tensors("traps", torch.float64)
    e = R.edges_of(f)
    assert (e[:, 0] == e[:, 1]).any()
    V = len(v)
    ii, jj = f[:, [1, 2, 0]].flatten(), f[:, [2, 0, 1]].flatten()                                    # the dense operator, entry by entry
    L = torch.zeros((V, V), dtype=torch.float64)
    for i, j in set(zip(torch.cat([ii, jj]).tolist(), torch.cat([jj, ii]).tolist())):
        L[i, j] -= 1.0
        L[i, i] += 1.0
    assert torch.allclose((L @ v).norm(dim=1).mean(), R.laplacian(v, e), rtol=0, atol=ROUND_OFF)


@pytest.mark.parametrize("name", ["kuhn_8", "traps"])
@pytest.mark.parametrize("what", ["normals", "consistency", "consistency_of_normals", "laplacian"])
def test_autograd_agrees_with_central_differences(name, what):
    v0, faces = R.tensors(name, torch.float64)
    e = R.edges_of(faces)
    gn = torch.tensor(R.upstream(name, "random")).double()
    if what == "consistency":
        v0 = R.vertex_normals(v0, faces) * 1.25                                                      # (not unit length: the norms' derivative takes part)
    fn = {"normals": lambda v: (R.vertex_normals(v, faces) * gn).sum(), "consistency": lambda v: R.normal_consistency(v, e),
          "consistency_of_normals": lambda v: R.mesh_normal_consistency(v, faces, e), "laplacian": lambda v: R.laplacian(v, e)}[what]
    v = v0.clone().requires_grad_(True)
    fn(v).backward()
    rng = np.random.default_rng(17)
    h = 1e-8                                                                                         # kuhn_8 has slivers whose normal sum is 6e-6 long: the step stays far below that
    for _ in range(6):                                                                               # directional derivatives along random directions
        d = torch.tensor(rng.uniform(-1.0, 1.0, tuple(v0.shape)))
        fd = (fn(v0 + h * d) - fn(v0 - h * d)) / (2 * h)
        an = (v.grad * d).sum()
        assert abs(float(fd - an)) <= 1e-6 * max(1.0, abs(float(an))), (name, what, float(fd), float(an))


def test_no_comparison_rests_on_a_coin_toss():
    for name in R.SCENES:
        sq, ratio = R.row_figures(name)
        fin = np.isfinite(sq)
        assert fin.all() or name == "fan"
        if name != "kuhn_32_small":
            live = fin & (sq != 0)
            assert (sq[live] >= 2e-20).all() and (ratio[live] >= 0.05).all(), (name, sq[live].min(), ratio[live].min())
            assert not R.left_out(name).any()
    sq, _ = R.row_figures("kuhn_32_small")
    assert 0 < int(R.left_out("kuhn_32_small").sum()) <= 2
    assert int((sq <= R.NORMAL_EPS).sum()) == R.KUHN_32_SMALL_DEFAULT_ROWS
    n64 = R.reference("kuhn_32_small", "normals")[0][0]
    assert np.array_equal(n64[sq <= R.NORMAL_EPS], np.tile([0.0, 0.0, 1.0], (R.KUHN_32_SMALL_DEFAULT_ROWS, 1)))
    assert (np.isnan(R.scene("fan")["v_pos"]).all(axis=1)).sum() == 3                                # three NaN vertices
    m = R.scene("umbrella")
    assert np.bincount(m["faces"].reshape(-1)).max() == 300 and len(m["faces"]) == 300
    t = R.scene("traps")
    assert len(t["faces"]) == 20 and 11 not in t["faces"]
    assert len(R.scene("kuhn_32")["v_pos"]) == 8260 and len(R.scene("kuhn_32")["faces"]) == 16516 and len(R.edges_of(torch.tensor(R.scene("kuhn_32")["faces"]))) == 24774
