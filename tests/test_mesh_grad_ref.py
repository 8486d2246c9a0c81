"""CPU: the gradient reference (tests/mesh_grad_ref.py) against itself -- its decisions against tests/mesh_aa_ref.py's output, its autograd against
central finite differences in float64, and the non-vacuity of the scenes the GPU tests use.

Finite differences: step h = 1e-6 max(1, |coordinate|), so the truncation error h^2 f''' / 6 is ~1e-12 f''' and the roundoff 2^-52 |L| / h is
~1e-8 for the |L| of a few hundred that a vertex's pixels add up to; the bar is 1e-6 of the gradient's largest magnitude plus 1e-6.  L is
evaluated over the vertex's own pixels or pairs only (the rest does not move).  A coordinate whose perturbation changes an integer decision
-- a snapped coordinate for antialias, a clamp's state for u, v -- is excluded, and most must remain."""
import numpy as np
import pytest
import torch

from tests import mesh_aa_ref as A
from tests import mesh_grad_ref as G
from tests import mesh_ref as M

FD_SCENES = ("ball_96", "patch_97x61")
STEP = 1e-6


def _fd_bar(grad):
    return 1e-6 * float(np.abs(grad).max()) + 1e-6


@pytest.mark.parametrize("name", G.AA_GRAD_SCENES)
def test_the_recomputed_pair_decisions_give_the_antialias_reference(name):
    """aa_pairs + aa_torch reproduce tests/mesh_aa_ref.py's out64 and out32: the decisions it keeps to itself are recomputed correctly"""
    s, C = G.scene(name), 3
    ref = A.reference(name, C)
    g = np.zeros((s["H"], s["W"], C), np.float32)
    for dtype, key in ((torch.float64, "out64"), (torch.float32, "out32")):
        mine = G.antialias_grads(dtype, A.colors(name, C), G.scene_rast(name), s["pos"], s["tri"], A.scene_topology(name), g)
        assert len(mine["pairs"]["R"]) == ref["n_contrib"]
        assert np.array_equal(mine["out"], ref[key].astype(np.float64)), (name, key)
    pr = mine["pairs"]
    assert int((pr["sign"] > 0).sum()) == ref["n_pos"] and int(pr["horiz"].sum()) == ref["n_horizontal"]
    touched = np.zeros(s["H"] * s["W"], bool)
    touched[pr["R"]] = True
    assert np.array_equal(touched.reshape(s["H"], s["W"]), ref["touched"])


@pytest.mark.parametrize("name", G.RAST_SCENES)
def test_uv_gradient_scenes_are_not_vacuous(name):
    """few covered pixels sit at a clamp bound (they get a zero upstream in the tests; no output is excluded)"""
    s = G.scene(name)
    amb, n = G.uv_ambiguous(s["pos"], s["tri"], G.scene_rast(name))
    print(f"{name}: {int(amb.sum())} of {n} covered pixels within 4 eta of a clamp bound ({amb.sum() / max(n, 1):.4f})")
    assert n > 0 and amb.sum() <= M.AMBIGUOUS_CAP * n


@pytest.mark.parametrize("name", A.NON_VACUOUS)
def test_silhouette_gradient_scenes_are_not_vacuous(name):
    s = G.scene(name)
    rast = G.scene_rast(name)
    pr = G.aa_pairs(rast, s["pos"], s["tri"], A.scene_topology(name))
    n_covered = int((rast[..., 3] > 0).sum())
    assert len(np.unique(pr["R"])) >= 0.01 * n_covered
    assert (pr["sign"] > 0).any() and (pr["sign"] < 0).any() and pr["horiz"].any() and (~pr["horiz"]).any()


def _pos64(s):
    return np.asarray(s["pos"], np.float32).astype(np.float64)


@pytest.mark.parametrize("name", FD_SCENES)
def test_uv_gradient_against_finite_differences(name):
    s = G.scene(name)
    rast, H, W = G.scene_rast(name), s["H"], s["W"]
    amb, _ = G.uv_ambiguous(s["pos"], s["tri"], rast)
    g = G.upstream(name, (H, W, 4), "fd_uv", smooth=True)
    g[amb] = 0.0
    ref = G.rasterize_grads(torch.float64, s["pos"], s["tri"], rast, g)["d_pos"]
    assert not ref[:, 2].any() and np.abs(ref).max() > 0
    pix, vid = G.covered(rast, s["tri"], len(s["pos"]))
    gp = torch.tensor(g.reshape(-1, 4)[pix], dtype=torch.float64)
    i, j = torch.from_numpy(pix % W), torch.from_numpy(pix // W)
    pos = _pos64(s)

    def value(p, rows):
        with torch.no_grad():
            u, v, u0, v0 = G.uv_torch(torch.from_numpy(p[vid[rows]]), i[rows], j[rows], W, H)
        live = (gp[rows, :2] != 0).any(dim=1)
        state = torch.stack([u0 < 0, u0 > 1, v0 < 0, v0 > 1, u0.clamp(0, 1) + v0.clamp(0, 1) >= 1])[:, live]
        return float((u * gp[rows, 0] + v * gp[rows, 1]).sum()), state

    checked = skipped = 0
    for k in np.unique(vid):
        rows = np.nonzero((vid == k).any(axis=1))[0]
        _, base = value(pos, rows)
        for c in range(4):
            h = STEP * max(1.0, abs(pos[k, c]))
            up, dn = pos.copy(), pos.copy()
            up[k, c] += h; dn[k, c] -= h
            (lu, su), (ld, sd) = value(up, rows), value(dn, rows)
            if not (torch.equal(su, base) and torch.equal(sd, base)):
                skipped += 1
                continue
            checked += 1
            assert abs((lu - ld) / (2 * h) - ref[k, c]) <= _fd_bar(ref), (name, int(k), c, (lu - ld) / (2 * h), ref[k, c])
    unseen = np.setdiff1d(np.arange(len(pos)), np.unique(vid))
    assert not ref[unseen].any()
    assert checked >= 0.9 * (checked + skipped) and checked > 100, (checked, skipped)


@pytest.mark.parametrize("name", FD_SCENES)
def test_antialias_gradients_against_finite_differences(name):
    s, C = G.scene(name), 3
    rast, H, W = G.scene_rast(name), s["H"], s["W"]
    color, topo = A.colors(name, C), A.scene_topology(name)
    g = G.upstream(name, (H, W, C), "fd_aa", smooth=True)
    ref = G.antialias_grads(torch.float64, color, rast, s["pos"], s["tri"], topo, g)
    pr, d_pos = ref["pairs"], ref["d_pos"]
    assert not d_pos[:, 2].any() and np.abs(d_pos).max() > 0
    ct, gt = torch.tensor(color.reshape(-1, C), dtype=torch.float64), torch.tensor(g.reshape(-1, C), dtype=torch.float64)
    pos = _pos64(s)
    X0, Y0, ok0, _, _ = M.snap(pos, W, H)

    def value(p, rows):
        sub = {k: v[rows] for k, v in pr.items()}
        with torch.no_grad():
            out = G.aa_torch(ct, torch.from_numpy(p[sub["va"]]), torch.from_numpy(p[sub["vb"]]), sub, W, H, real=True)
        return float(((out - ct) * gt).sum())

    used = np.unique(np.concatenate([pr["va"], pr["vb"]]))
    checked = skipped = 0
    for k in used:
        rows = np.nonzero((pr["va"] == k) | (pr["vb"] == k))[0]
        for c in range(4):
            h = STEP * max(1.0, abs(pos[k, c]))
            up, dn = pos.copy(), pos.copy()
            up[k, c] += h; dn[k, c] -= h
            same = all(np.array_equal(a, b) for q in (up, dn) for a, b in zip(M.snap(q, W, H)[:3], (X0, Y0, ok0)))
            if not same:                                                          # the perturbation moves a snapped coordinate: a decision may change
                skipped += 1
                continue
            checked += 1
            fd = (value(up, rows) - value(dn, rows)) / (2 * h)
            assert abs(fd - d_pos[k, c]) <= _fd_bar(d_pos), (name, int(k), c, fd, d_pos[k, c])
    assert not d_pos[np.setdiff1d(np.arange(len(pos)), used)].any()
    assert checked >= 0.9 * (checked + skipped) and checked >= 4 * 12, (checked, skipped)       # a dozen silhouette vertices at least
    # color: out is linear in it, so a finite difference along a random direction is exact up to roundoff
    rng = np.random.default_rng(5)
    direction = torch.tensor(rng.uniform(-1, 1, ct.shape))
    PA, PB = torch.from_numpy(pos[pr["va"]]), torch.from_numpy(pos[pr["vb"]])
    with torch.no_grad():
        lu = float((G.aa_torch(ct + 0.5 * direction, PA, PB, pr, W, H) * gt).sum())
        ld = float((G.aa_torch(ct - 0.5 * direction, PA, PB, pr, W, H) * gt).sum())
    assert abs((lu - ld) - float((torch.tensor(ref["d_color"].reshape(-1, C)) * direction).sum())) <= 1e-9 * max(1.0, abs(lu))


def test_interpolate_gradients_against_finite_differences():
    name, C = "hand_33x17", 3
    s = G.scene(name)
    rast = G.scene_rast(name)
    H, W = rast.shape[:2]
    rng = np.random.default_rng(9)
    attr = rng.uniform(-1, 1, (len(s["pos"]), C)).astype(np.float32)
    g = G.upstream(name, (H, W, C), "fd_interp", smooth=True)
    ref = G.interpolate_grads(torch.float64, attr, rast, s["tri"], g)
    pix, vid = G.covered(rast, s["tri"], len(attr))
    assert not ref["d_rast"][..., 2:].any() and not ref["d_rast"].reshape(-1, 4)[np.setdiff1d(np.arange(H * W), pix)].any()
    gt, uv = torch.tensor(g.reshape(-1, C)[pix], dtype=torch.float64), torch.tensor(rast.reshape(-1, 4)[pix][:, :2], dtype=torch.float64)
    value = lambda a, q: float((G.interpolate_torch(torch.from_numpy(a)[torch.from_numpy(vid).reshape(-1)].reshape(-1, 3, C), q) * gt).sum())
    a64 = attr.astype(np.float64)
    for d_attr_dir in (rng.uniform(-1, 1, a64.shape),):                           # linear in attr and in (u, v): a unit step is exact up to roundoff
        fd = value(a64 + 0.5 * d_attr_dir, uv) - value(a64 - 0.5 * d_attr_dir, uv)
        assert abs(fd - float((ref["d_attr"] * d_attr_dir).sum())) <= 1e-9 * max(1.0, abs(fd))
    duv = torch.tensor(rng.uniform(-1, 1, tuple(uv.shape)))
    fd = value(a64, uv + 0.5 * duv) - value(a64, uv - 0.5 * duv)
    assert abs(fd - float((torch.tensor(ref["d_rast"].reshape(-1, 4)[pix][:, :2]) * duv).sum())) <= 1e-9 * max(1.0, abs(fd))


def test_fixed_point_term():
    assert G.fixed_point_term(0.0, 10) == 0.0 and G.fixed_point_term(1.0, 0) == 0.0
    assert G.fixed_point_term(0.75, 1) == 2.0 ** -35 and G.fixed_point_term(1.0, 4) == 4 * 2.0 ** -34        # 2^(e-1) <= B < 2^e
    assert G.fixed_point_term(3.0, 1 << 18) == 2.0 ** (18 + 2 - 35)
