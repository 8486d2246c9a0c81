"""The feature-channel output of the rasterizer (feature_map[c] = sum_i T_i alpha_i features[i, c] over the pairs the colour frame blended) and
its gradients, on the device.

Yardstick (tests/test_features_abi.py checks it on the CPU): per channel triple, the oracle's frame of the same geometry with
colors_precomp = F[:, triple] (zero-padded), no SH and background 0 is the feature map's triple; under the upstream g[triple] its dL_dcolors
is dL_dfeatures[:, triple] and the sum over the triples of its other gradients is the through-alpha share.  For the upstream
(dL_dpix, g_A, g_D, g_F) the expectation is that share plus the colour, alpha and depth terms of tests/test_gpu_depth.py.

Bar: the project's frozen one, computed here from the reference alone -- per tensor min(max(1e-4, 2 eta), 1e-3) with
eta = rel_l2(that expectation from the fp32 oracle, the same from the fp64 oracle), dL_dfeatures included.  No failure budget.
Scenes, kernel modes and helpers are those of tests/test_gpu_alpha.py / tests/test_gpu_depth.py; every scene runs with C = 5 (one group,
narrow and wide kernel slots both partly filled), and g13_dense_2k and cloud_6000_classes with C = 1, 8, 9, 16 as well (a single channel, a
full group, a group plus one, the maximum)."""
import functools

import numpy as np
import pytest
import torch

from tests import test_gpu_alpha as A
from tests import test_gpu_depth as D
from tests import util
from tests.test_features_abi import make_features, oracle_features

pytestmark = pytest.mark.gpu

SCENES, MODES, SUMMED, COLOUR_ONLY, LEAVES = A.SCENES, A.MODES, A.SUMMED, A.COLOUR_ONLY, A.LEAVES
NAMES = A.NAMES + ("dL_dfeatures",)
CASES = [(n, 5) for n in SCENES] + [(n, C) for n in ("g13_dense_2k", "cloud_6000_classes") for C in (1, 8, 9, 16)]
check_gradients, _t = A.check_gradients, A._t
KEYS = SUMMED + COLOUR_ONLY + ("dL_dfeatures",)
deterministic_default = A.deterministic_default


@functools.lru_cache(maxsize=None)
def scene(name, C):
    """-> the depth suite's scene (inputs, upstreams, colour / alpha / depth terms) plus the features, their upstream, the yardstick's map and,
    per oracle build, the feature term of the expectation and dL_dfeatures (computed once per case, read-only)"""
    d = D.scene(name)
    inp, H, W = d["inp"], d["H"], d["W"]
    P = int(np.asarray(inp["means3D"]).shape[0])
    F = make_features(P, C, seed=100 + C)
    g_F = (np.random.Generator(np.random.PCG64(5150 + C)).standard_normal((C, H, W)) / (H * W)).astype(np.float32)
    term, dF, fmap = {}, {}, None
    for variant in ("f32", "f64"):
        n_contrib = np.asarray(util.oracle_run(inp, None, variant=variant)["n_contrib"])
        m, dF[variant], term[variant] = oracle_features(inp, F, g_F, variant, n_contrib=n_contrib)
        if variant == "f32":
            fmap = np.asarray(m, np.float32)
    return dict(d, C=C, F=F, g_F=g_F, fmap=fmap, feat_term=term, dF=dF)


def expectation(s, colour: bool, alpha: bool, depth: bool) -> dict:
    """the feature term, plus the colour, alpha and depth terms on request -- for both oracle builds"""
    exp = {}
    for variant in ("f32", "f64"):
        e = {k: s["feat_term"][variant][k].copy() for k in SUMMED}
        e.update({k: np.zeros_like(s["colour"][variant][k]) for k in COLOUR_ONLY})
        e["dL_dfeatures"] = s["dF"][variant]
        if colour:
            for k in SUMMED + COLOUR_ONLY:
                e[k] = e[k] + s["colour"][variant][k]
        if alpha:
            for k in SUMMED:
                e[k] = e[k] + s["alpha_only"][variant][k]
        if depth:
            for k in SUMMED:
                e[k] = e[k] + s["depth_term"][variant][k]
        exp[variant] = e
    return exp


class Frame(D.Frame):
    def features(self, F):
        from diff_gaussian_rasterization import _C
        return _C.features_from_state(self.geom, self.binning, self.img, _t(F, self.dev), self.P, self.H, self.W, int(self.R))

    def backward(self, dL, g_A=None, g_D=None, g_F=None, F=None, **kw):
        from diff_gaussian_rasterization import _C
        if g_A is not None:
            kw["grad_out_alpha"] = _t(g_A, self.dev).reshape(1, self.H, self.W)
        if g_D is not None:
            kw["grad_out_depth"] = _t(g_D, self.dev).reshape(1, self.H, self.W)
        if g_F is not None:
            kw["grad_out_features"], kw["features"] = _t(g_F, self.dev), _t(F, self.dev)
        g = _C.rasterize_gaussians_backward(self.bg, self.means, self.radii, self.colors, self.scales, self.rots, self.sm, self.cov, self.view, self.proj, self.tfx,
                                            self.tfy, _t(dL, self.dev), self.sh, self.D, self.campos, self.geom, self.R, self.binning, self.img, False, _with_conic=True, **kw)
        assert len(g) == (10 if g_F is not None else 9)
        return {n: v.cpu().numpy() for n, v in zip(NAMES, g)}


# ---- forward ----
@pytest.mark.parametrize("name,C", CASES)
def test_feature_map_is_the_composited_feature_of_the_colour_frame(name, C, gpu_device):
    s = scene(name, C)
    H, W, F = s["H"], s["W"], s["F"]
    f = Frame(s["inp"], gpu_device)
    out = f.features(F)
    assert out.dtype == torch.float32 and tuple(out.shape) == (C, H, W)
    m = out.cpu().numpy()
    for c in range(C):
        e = util.rel_l2(m[c], s["fmap"][c])
        print(f"{name} C={C}: channel {c} against the oracle's feature-colour frame: rel-L2 {e:.3e}")
        assert e <= util.tolerance("color", None)
    assert np.array_equal(f.features(F).cpu().numpy(), m), "two runs over one frame's state differ"
    # exactly 0 on every pixel of a tile without instances
    rg = f.field("ranges").cpu().numpy().reshape(-1, 2)
    gx = (W + 15) // 16
    empty = 0
    for t in np.nonzero(rg[:, 1] == rg[:, 0])[0]:
        ty, tx = divmod(int(t), gx)
        assert np.all(m[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 0), f"tile {t} has no instance but the map != 0"
        empty += 1
    if name == "g10_all_culled":
        assert f.R == 0 and np.all(m == 0)
    else:
        assert m.min() < 0 < m.max(), "signed features, nothing clamped"
    if name == "cloud_600_sparse":
        assert empty > 0
    # permuting the feature columns permutes the channels bit for bit (reversal: at C = 16 every column changes its group of 8)
    perm = np.arange(C)[::-1].copy()
    assert np.array_equal(f.features(F[:, perm]).cpu().numpy(), m[perm]), "a channel's bits depend on its slot"
    if C > 1:                                               # ... and do not depend on how many channels travel with it
        assert np.array_equal(f.features(F[:, :1]).cpu().numpy()[0], m[0])
        assert np.array_equal(f.features(F[:, C - 1:]).cpu().numpy()[0], m[C - 1])
    # the same bits whatever forward wrote the state: light groups on / off, the speculative forward
    for kw in (dict(light_tiles=True), dict(light_tiles=False), dict(r_guess=max(int(f.R), 1) + 1000), dict(r_guess=max(int(f.R), 1) + 1000, light_tiles=True)):
        assert np.array_equal(Frame(s["inp"], gpu_device, **kw).features(F).cpu().numpy(), m), kw


@pytest.mark.parametrize("name", SCENES)
def test_a_column_of_ones_is_alpha_and_a_column_of_z_is_depth(name, gpu_device):
    """The same pairs as alpha and as tgs_depth.  alpha is fl(1 - T_final), the ones channel an fp32 sum of n_contrib products whose partial
    sums stay <= 1: each of the n + 2 roundings is at most 2^-24, doubled for both sides -- (n + 2) 2^-23; the z channel the same times
    max z (the slack form tests/test_gpu_depth.py derives)."""
    s = scene(name, 5)
    H, W = s["H"], s["W"]
    f = Frame(s["inp"], gpu_device)
    vis = s["radii"] > 0
    z = np.where(vis, f.field("depths").cpu().numpy().reshape(-1), 0.0).astype(np.float32)      # (a culled Gaussian's stored depth is never read)
    G = s["F"].copy()
    G[:, 1], G[:, 3] = 1.0, z
    m = f.features(G).cpu().numpy().astype(np.float64)
    n = f.field("n_contrib").cpu().numpy().reshape(H, W).astype(np.float64)
    alpha, depth = f.alpha().cpu().numpy()[0], f.depth().cpu().numpy()[0]
    da = np.abs(m[1] - alpha.astype(np.float64))
    print(f"{name}: ones channel against alpha: max abs {da.max():.3e}")
    assert np.all(da <= (n + 2.0) * 2.0 ** -23)
    zmax = float(z[vis].max()) if vis.any() else 0.0
    dd = np.abs(m[3] - depth.astype(np.float64))
    print(f"{name}: z channel against tgs_depth: max abs {dd.max():.3e}, bit-equal: {bool(np.array_equal(m[3].astype(np.float32), depth))}")
    assert np.all(dd <= (n + 2.0) * 2.0 ** -23 * zmax)


def test_feature_map_of_an_empty_model_and_the_output_order(gpu_device, monkeypatch):
    s = scene("cloud_600_sparse", 5)
    inp, F = s["inp"], s["F"]
    empty = dict(inp, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32), shs=np.zeros((0, 4, 3), np.float32))
    F0 = torch.zeros(0, 5, device=gpu_device)
    out = A._render(empty, gpu_device, A._leaves(empty, gpu_device), features=F0)
    assert len(out) == 3 and tuple(out[2].shape) == (5, 40, 72) and out[2].dtype == torch.float32 and bool((out[2] == 0).all()) and out[1].numel() == 0
    out = A._render(empty, gpu_device, A._leaves(empty, gpu_device), return_alpha=True, return_depth=True, features=F0)
    assert len(out) == 5 and tuple(out[4].shape) == (5, 40, 72) and all(bool((o == 0).all()) for o in out[2:])
    # (color, radii), then alpha, then depth, then the map: each the bits of the _C surface, through the plain and the speculative public forward
    f = Frame(inp, gpu_device)
    alpha, depth, fmap = f.alpha().cpu().numpy(), f.depth().cpu().numpy(), f.features(F).cpu().numpy()
    Ft = _t(F, gpu_device)
    import youreditableavatar_amd.diff_gaussian_rasterization as dgr
    with torch.no_grad():
        for _ in range(3):                                   # (the second and third call of a key speculate)
            color, radii, a, d, m = A._render(inp, gpu_device, A._leaves(inp, gpu_device), return_alpha=True, return_depth=True, features=Ft)
            assert np.array_equal(a.cpu().numpy(), alpha) and np.array_equal(d.cpu().numpy(), depth) and np.array_equal(m.cpu().numpy(), fmap)
        color, radii, d, m = A._render(inp, gpu_device, A._leaves(inp, gpu_device), return_depth=True, features=Ft)
        assert np.array_equal(d.cpu().numpy(), depth) and np.array_equal(m.cpu().numpy(), fmap)
        monkeypatch.setattr(dgr, "_SPECULATE", False)
        color, radii, m = A._render(inp, gpu_device, A._leaves(inp, gpu_device), features=Ft)
        assert np.array_equal(m.cpu().numpy(), fmap) and np.array_equal(color.cpu().numpy(), f.color.cpu().numpy())
        # a non-contiguous [P, C] view is taken contiguous
        m = A._render(inp, gpu_device, A._leaves(inp, gpu_device), features=Ft.t().contiguous().t())[2]
        assert np.array_equal(m.cpu().numpy(), fmap)
    for bad in (torch.zeros(Ft.shape[0], 17, device=gpu_device), torch.zeros(Ft.shape[0], 0, device=gpu_device), Ft.double(), Ft[:-1], Ft.cpu()):
        with pytest.raises(ValueError, match="features"):
            A._render(inp, gpu_device, A._leaves(inp, gpu_device), features=bad)


# ---- gradients through the _C surface ----
UPSTREAMS = {"features alone": (False, False, False), "colour + features": (True, False, False), "colour + alpha + depth + features": (True, True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,C", CASES)
def test_gradients_with_feature_upstream(name, C, mode, gpu_device):
    s = scene(name, C)
    fwd_kw, bwd_kw = MODES[mode]
    f = Frame(s["inp"], gpu_device, **fwd_kw)
    assert np.array_equal(f.radii.cpu().numpy(), s["radii"])
    vis = s["radii"] > 0
    for what, (colour, alpha, depth) in UPSTREAMS.items():
        dL = s["dL"] if colour else np.zeros_like(s["dL"])
        args = (dL, s["g_A"] if alpha else None, s["g_D"] if depth else None, s["g_F"], s["F"])
        g = f.backward(*args, **bwd_kw)
        assert g["dL_dfeatures"].shape == s["F"].shape
        check_gradients(g, expectation(s, colour, alpha, depth), f"{name} C={C} [{mode}] {what}", keys=KEYS)
        assert np.all(g["dL_dmeans2D"][:, 2] == 0)
        for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dfeatures"):
            assert np.all(g[k][~vis] == 0), f"{k}: culled Gaussians must have zero gradient"
        if not colour:
            assert not np.any(g["dL_dsh"]) and not np.any(g["dL_dcolors"]), "the feature map does not depend on the colours"
        if mode == "deterministic":
            again = f.backward(*args, **bwd_kw)
            for k in NAMES:
                assert np.array_equal(g[k], again[k]), f"{k}: two deterministic backward passes of one frame differ"


@pytest.mark.parametrize("C", (5, 16))
def test_backward_without_the_keyword_is_the_depth_call(C, gpu_device):
    """grad_out_features=None launches no feature kernel: the bits of the call without the keyword, whatever other upstreams travel; a zero
    upstream through the feature kernels (two launches at C = 16) adds zeros -- x + 0 = x, and the conic shares are split into hi + lo again,
    which keeps hi + lo's double value -- so the other gradients keep their bits in deterministic mode, and dL_dfeatures is all zero."""
    s = scene("g13_dense_2k", C)
    f = Frame(s["inp"], gpu_device)
    for g_A, g_D in ((None, None), (s["g_A"], None), (s["g_A"], s["g_D"])):
        a, b = D.Frame.backward(f, s["dL"], g_A, g_D, deterministic=True), f.backward(s["dL"], g_A, g_D, None, None, deterministic=True)
        z = f.backward(s["dL"], g_A, g_D, np.zeros_like(s["g_F"]), s["F"], deterministic=True)
        for k in A.NAMES:
            assert np.array_equal(a[k], b[k]), k
            assert np.array_equal(a[k], z[k]), k
        assert "dL_dfeatures" not in b and not np.any(z["dL_dfeatures"])
    Ft = _t(s["F"], gpu_device)
    for bad in (dict(grad_out_features=torch.zeros(C, 3, 3, device=gpu_device), features=Ft),
                dict(grad_out_features=torch.zeros(C + 1, s["H"], s["W"], device=gpu_device), features=Ft),
                dict(grad_out_features=torch.zeros(C, s["H"], s["W"], device=gpu_device), features=Ft[:-1]),
                dict(grad_out_features=torch.zeros(C, s["H"], s["W"], device=gpu_device)),
                dict(grad_out_features=torch.zeros(17, s["H"], s["W"], device=gpu_device), features=torch.zeros(f.P, 17, device=gpu_device))):
        with pytest.raises(RuntimeError, match="grad_out_features"):
            f.backward(s["dL"], None, None, **bad)


# ---- the public API ----
def _leaves(s, dev, feature_grad=True):
    L = A._leaves(s["inp"], dev)
    L["features"] = _t(s["F"], dev).requires_grad_(feature_grad)
    return L


def _render(s, dev, L, **kw):
    return A._render(s["inp"], dev, L, features=L["features"], **kw)


def _as_exp(L):
    g = {LEAVES[k]: v for k, v in A._grads(L).items()}
    g["dL_dfeatures"] = None if L["features"].grad is None else L["features"].grad.detach().cpu().numpy()
    return g


def test_an_unused_feature_map_changes_nothing(gpu_device, deterministic_default):
    s = scene("cloud_600_sparse", 5)
    inp, dev = s["inp"], gpu_device
    w = _t(s["dL"], dev)
    L0 = A._leaves(inp, dev)
    out = A._render(inp, dev, L0)
    assert isinstance(out, tuple) and len(out) == 2 and type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBackward")
    (w * out[0]).sum().backward()
    g0 = A._grads(L0)
    # colour alone with a feature map returned (unused: no feature gradient reaches the node): bit-identical to the plain node
    for kw in (dict(), dict(return_depth=True), dict(return_alpha=True, return_depth=True)):
        L1 = _leaves(s, dev)
        res = _render(s, dev, L1, **kw)
        assert len(res) == 3 + len(kw) and res[-1].requires_grad and not res[1].requires_grad and tuple(res[-1].shape) == (5, s["H"], s["W"])
        (w * res[0]).sum().backward()
        g1 = A._grads(L1)
        for leaf in LEAVES:
            assert np.array_equal(g0[leaf], g1[leaf]), (leaf, kw)
        assert L1["features"].grad is None


def test_feature_terms_through_autograd(gpu_device):
    s = scene("cloud_600_sparse", 5)
    dev, H, W = gpu_device, s["H"], s["W"]
    wF, wD, wA, wC = _t(s["g_F"], dev), _t(s["g_D"], dev).reshape(1, H, W), _t(s["g_A"], dev).reshape(1, H, W), _t(s["dL"], dev)
    # features alone: the image is unused, the colour gradient is absent
    L = _leaves(s, dev)
    color, radii, fmap = _render(s, dev, L)
    (wF * fmap).sum().backward()
    g = _as_exp(L)
    assert not np.any(g.pop("dL_dsh")), "the feature map does not depend on the colours"
    check_gradients(g, expectation(s, False, False, False), "features alone", keys=SUMMED + ("dL_dfeatures",))
    # colour + features in one loss
    L = _leaves(s, dev)
    color, radii, fmap = _render(s, dev, L)
    ((wC * color).sum() + (wF * fmap).sum()).backward()
    check_gradients(_as_exp(L), expectation(s, True, False, False), "colour + features", keys=KEYS)
    # all four outputs in one loss, in the documented order
    L = _leaves(s, dev)
    color, radii, alpha, depth, fmap = _render(s, dev, L, return_alpha=True, return_depth=True)
    assert tuple(alpha.shape) == (1, H, W) and tuple(depth.shape) == (1, H, W) and tuple(fmap.shape) == (5, H, W)
    assert float(alpha.max()) <= 1.0 < float(depth.max()) and float(fmap.min()) < 0
    ((wC * color).sum() + (wA * alpha).sum() + (wD * depth).sum() + (wF * fmap).sum()).backward()
    check_gradients(_as_exp(L), expectation(s, True, True, True), "colour + alpha + depth + features", keys=KEYS)
    # features that need no gradient: none comes back, the other gradients still hold the through-alpha share
    L = _leaves(s, dev, feature_grad=False)
    color, radii, fmap = _render(s, dev, L)
    assert fmap.requires_grad
    ((wC * color).sum() + (wF * fmap).sum()).backward()
    g = _as_exp(L)
    assert g.pop("dL_dfeatures") is None
    check_gradients(g, expectation(s, True, False, False), "colour + features, features without a gradient")
    # depth used, the map returned and unused: the depth suite's expectation
    L = _leaves(s, dev)
    color, radii, depth, fmap = _render(s, dev, L, return_depth=True)
    ((wC * color).sum() + (wD * depth).sum()).backward()
    g = _as_exp(L)
    assert g.pop("dL_dfeatures") is None
    check_gradients(g, D.expectation(s, True, False), "colour + depth, the map unused")


def test_example_fits_feature_maps(gpu_device):
    """examples/fit_features.py: l1(feature_map, target) through features= and autograd, Adam on a 4-channel feature and the opacities; the loss falls."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fit_features", os.path.join(util.ROOT, "examples", "fit_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    vals = mod.run(steps=12, P=1500, W=96, H=64, log=lines.append)
    print("\n".join(lines))
    assert len(vals) == 13 and all(np.isfinite(vals)) and vals[-1] < vals[0]
