"""CPU: the marching-tetrahedra restatement (tests/mt_ref.py) against what the reference's own ``_forward`` returned
(tests/golden/ref_mt_fixture.npz, recorded by tests/make_ref_mt_fixture.py), against central finite differences in float64, and the
closed-manifold property of the Kuhn-grid scenes the GPU tests use.

Finite differences, as tests/test_mesh_grad_ref.py takes them: step h = 1e-6 max(1, |coordinate|), bar 1e-6 of the gradient's largest magnitude
plus 1e-6.  The smallest |sdf| on a crossing edge of kuhn_8 is 4e-4, far above h, so no perturbation changes a sign: every coordinate is
checked and none is left out."""
import numpy as np
import pytest
import torch

from tests import mt_ref as R

STEP = 1e-6


@pytest.mark.parametrize("name", R.FIXTURE_SCENES)
def test_the_restatement_reproduces_the_recorded_reference(name):
    fx = R.fixture()
    s = R.scene(name)
    for k in ("pos", "sdf", "tet"):                                          # the scene the fixture was recorded on is the scene the tests build
        assert np.array_equal(fx[f"{name}.{k}"], s[k], equal_nan=True), (name, k)
    for got in R.reference(name):                                            # float64 and float32: the integers do not depend on the precision
        for k in R.KEYS[1:]:
            want = fx[f"{name}.{k}"]
            want = want.reshape(-1, 2) if k == "interp_v" else want          # (the reference keeps a singleton axis in front of the pair: [M,1,2])
            assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (name, k)
    got, want = R.reference(name)[0]["verts"], fx[f"{name}.verts"]
    assert want.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.astype(np.float32), want.astype(np.float32), equal_nan=True)      # float32 rounding of the float64 value
    n_nan = int(np.isnan(want).any(axis=1).sum())
    assert (n_nan == 3) if name == "fan" else (n_nan == 0)


def test_the_scenes_pin_what_they_are_meant_to_pin():
    c, f = R.scene("cases16"), R.scene("fan")
    occ = c["sdf"][c["tet"]] > 0
    assert np.array_equal((occ * (1 << np.arange(4))).sum(1), np.arange(16))                    # one tetrahedron per case code
    out = R.reference("cases16")[0]
    assert (np.diff(out["face_to_tet_idx"][:8]) > 0).all() and len(out["faces"]) == 8 + 2 * 6    # the ones, ascending, then the twos
    assert np.array_equal(out["face_to_tet_idx"][8:], np.repeat([3, 5, 6, 9, 10, 12], 2))
    assert (f["sdf"] == 0).sum() == 1 and np.isnan(f["sdf"]).sum() == 1
    assert len(np.unique(f["tet"], axis=0)) == len(f["tet"]) - 2 and (f["tet"][:, 0] == f["tet"][:, 1]).sum() == 1
    fan = R.reference("fan")[0]
    assert fan["valid_tets"].all() and len(fan["interp_v"]) < 6 * len(f["tet"])
    assert (fan["interp_v"][:, 0] < fan["interp_v"][:, 1]).all()


@pytest.mark.parametrize("name,counts", [("kuhn_8", (840, 544, 1084)), ("kuhn_32", (12632, 8260, 16516))])
def test_the_kuhn_meshes_are_closed_and_consistently_oriented(name, counts):
    out = R.reference(name)[0]
    assert (int(out["valid_tets"].sum()), len(out["verts"]), len(out["faces"])) == counts
    m = R.manifold_counts(out["faces"], len(out["verts"]))
    assert m == dict(directed_repeated=0, undirected_not_two=0, euler=2, unused_verts=0), m
    iv = out["interp_v"]
    key = iv[:, 0] * (1 << 32) + iv[:, 1]
    assert (np.diff(key) > 0).all()                                                              # ascending (min, max), no edge twice
    cell = 1.0 / int(name.split("_")[1])
    smallest = R.min_abs_sdf_on_crossing(R.scene(name), iv)
    print(f"{name}: smallest |sdf| on a crossing edge {smallest:.3g}, cell {cell:.3g}")
    assert smallest > 1e-6 * cell                                                                # the gradient tests' condition on the inputs


def test_autograd_against_finite_differences_on_kuhn_8():
    s = R.scene("kuhn_8")
    pos = torch.tensor(s["pos"]).double().requires_grad_(True)
    sdf = torch.tensor(s["sdf"]).double().requires_grad_(True)
    tet = torch.tensor(s["tet"])
    out = R.marching_tets(pos, sdf, tet)
    g = torch.tensor(np.random.default_rng(81).uniform(-1.0, 1.0, tuple(out["verts"].shape)))
    (out["verts"] * g).sum().backward()
    d_pos, d_sdf = pos.grad.numpy(), sdf.grad.numpy()
    iv = out["interp_v"]
    touched = np.zeros(len(s["pos"]), bool)
    touched[iv.numpy().reshape(-1)] = True
    assert 0 < touched.sum() < len(touched)
    assert not d_pos[~touched].any() and not d_sdf[~touched].any() and d_pos[touched].any(axis=1).all() and (d_sdf[touched] != 0).all()

    p0, s0 = pos.detach().numpy().copy(), sdf.detach().numpy().copy()

    def value(p, sd, whole):
        with torch.no_grad():
            if whole:                                                        # the whole restatement: the integer outputs must not have moved
                o = R.marching_tets(torch.from_numpy(p), torch.from_numpy(sd), tet)
                assert torch.equal(o["interp_v"], iv)
                return float((o["verts"] * g).sum())
            return float((R.vertices_of(torch.from_numpy(p), torch.from_numpy(sd), iv) * g).sum())

    checked = 0
    for v in np.nonzero(touched)[0]:
        whole = checked % 40 == 0                                            # (every coordinate on the fixed edges; one vertex in ten through all of it)
        for c in range(4):
            base = s0[v] if c == 3 else p0[v, c]
            h = STEP * max(1.0, abs(base))
            up_p, dn_p, up_s, dn_s = p0.copy(), p0.copy(), s0.copy(), s0.copy()
            if c == 3:
                up_s[v] += h; dn_s[v] -= h
            else:
                up_p[v, c] += h; dn_p[v, c] -= h
            fd = (value(up_p, up_s, whole) - value(dn_p, dn_s, whole)) / (2 * h)
            ref = d_sdf[v] if c == 3 else d_pos[v, c]
            bar = 1e-6 * float(np.abs(d_sdf if c == 3 else d_pos).max()) + 1e-6
            assert abs(fd - ref) <= bar, (int(v), c, fd, ref, bar)
            checked += 1
    assert checked == 4 * int(touched.sum())
