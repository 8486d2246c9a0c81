"""The accumulated-alpha output of the rasterizer (alpha = 1 - final_T) and its gradients, on the device.

Yardstick (tests/test_alpha_abi.py checks it on the CPU): the reference has no alpha output, but the same geometry rendered with colours 0
over the background (1, 0, 0) has channel 0 == final_T, so with the upstream gradient (-g_A, 0, 0) its gradients are exactly the gradients of
alpha under the upstream g_A.  By linearity, a frame with upstream (dL_dpix, g_A) must give
    oracle(inp, dL_dpix) + oracle(zero-colour inp, (-g_A, 0, 0))
for dL_dmeans2D, dL_dconic, dL_dopacity, dL_dmeans3D and dL_dscales + dL_drotations / dL_dcov3D, and the first run's values alone for
dL_dsh / dL_dcolors.

Bar: the project's frozen one, computed here from the reference alone -- per tensor min(max(1e-4, 2 eta), 1e-3) with
eta = rel_l2(that expectation from the fp32 oracle, the same from the fp64 oracle).  No failure budget: every scene, every tensor, against
the fp32 expectation.

Scenes: the smallest that reach every path of the per-pixel backward -- image edges inside tiles (g02), cov3D_precomp with SH and with
precomputed colours (g04, g05), early termination and a list longer than one 384-entry round (g08, g13), one splat on every tile (g09), no
instance at all (g10), and three seeded clouds with light (< 128 instances), mid and heavy (>= 1024) tiles side by side, near-opaque splats,
and a sparse frame with many empty tiles."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_alpha_abi import alpha_upstream, zero_colour_input

pytestmark = pytest.mark.gpu

FIXTURES = ("g02_sh0_nonmult16", "g04_sh2_cov3d", "g05_precomp_cov3d", "g08_opaque_termination", "g09_giant_splat", "g10_all_culled", "g13_dense_2k")
CLOUDS = ("cloud_6000_classes", "cloud_1500_opaque", "cloud_600_sparse")
SCENES = FIXTURES + CLOUDS
SUMMED = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")      # colour + alpha expectation
COLOUR_ONLY = ("dL_dsh", "dL_dcolors")                                                                              # alpha does not depend on them
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dconic")
BAR_CAP = util.BAR_CAP


def _input(name):
    from youreditableavatar_amd import scenes
    if name in FIXTURES:
        inp, _ = util.load_golden(name)
        return {k: v for k, v in inp.items() if k != "dL_dout_color"}
    if name == "cloud_6000_classes":
        return util.scene_input(scenes.make_cloud(6000, 0, 11, scale_mult=4.0), scenes.orbit_camera(50, 40, azimuth_deg=220, bg=(0.3, 0.6, 0.1)))
    if name == "cloud_1500_opaque":
        cloud = scenes.make_cloud(1500, 0, 13, scale_mult=8.0)
        cloud["opacities"] = np.full_like(cloud["opacities"], 0.99)
        return util.scene_input(cloud, scenes.orbit_camera(40, 24, azimuth_deg=260))
    return util.scene_input(scenes.make_cloud(600, 1, 1), scenes.orbit_camera(72, 40, azimuth_deg=30))


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> inputs, the two upstream gradients, and the expectation from the fp32 and the fp64 oracle (computed once per scene, read-only)"""
    from youreditableavatar_amd import scenes
    inp = _input(name)
    H, W = int(inp["image_height"]), int(inp["image_width"])
    dL = scenes.upstream_gradient(W, H)
    g_A = (np.random.Generator(np.random.PCG64(2024)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    zinp, dZ = zero_colour_input(inp), alpha_upstream(g_A)
    exp, alpha_only, ref = {}, {}, None
    for variant in ("f32", "f64"):
        a, z = util.oracle_run(inp, dL, variant=variant), util.oracle_run(zinp, dZ, variant=variant)
        e = {k: np.asarray(a[k], np.float64) + np.asarray(z[k], np.float64) for k in SUMMED}
        e.update({k: np.asarray(a[k], np.float64) for k in COLOUR_ONLY})
        exp[variant] = e
        alpha_only[variant] = {k: np.asarray(z[k], np.float64) for k in SUMMED}
        if variant == "f32":
            ref = a
    return dict(inp=inp, H=H, W=W, dL=dL, g_A=g_A, exp=exp, alpha_only=alpha_only, final_T=np.asarray(ref["final_T"], np.float32), radii=np.asarray(ref["radii"]))


def bar(e32, e64) -> float:
    return min(max(util.REL_TOL, 2.0 * util.rel_l2(e32, e64)), BAR_CAP)


def check_gradients(got: dict, exp: dict, what: str, keys=SUMMED + COLOUR_ONLY):
    worst = 0.0
    for k in keys:
        if k not in got:
            continue
        e32, e64 = exp["f32"][k], exp["f64"][k]
        a = np.asarray(got[k], np.float64).reshape(e32.shape)
        e, b = util.rel_l2(a, e32), bar(e32, e64)
        print(f"{what} {k}: rel-L2 {e:.3e} (bar {b:.2e}, eta {util.rel_l2(e32, e64):.2e}, to fp64 {util.rel_l2(a, e64):.3e})")
        worst = max(worst, e / b)
        assert e <= b, f"{what}: {k} rel-L2 {e:.3e} > {b:.2e}"
    return worst


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


class Frame:
    """One forward of a scene through the _C surface; alpha and backward passes on its state."""

    def __init__(self, inp, dev, **fwd_kw):
        from diff_gaussian_rasterization import _C
        t = lambda k: _t(inp[k], dev) if inp.get(k) is not None else torch.Tensor([])
        self.bg, self.means, self.opac, self.view, self.proj, self.campos = t("bg"), t("means3D"), t("opacities"), t("viewmatrix"), t("projmatrix"), t("campos")
        self.sh, self.colors, self.scales, self.rots, self.cov = t("shs"), t("colors_precomp"), t("scales"), t("rotations"), t("cov3D_precomp")
        self.H, self.W, self.D = int(inp["image_height"]), int(inp["image_width"]), int(inp["sh_degree"])
        self.sm, self.tfx, self.tfy = float(inp.get("scale_modifier", 1.0)), float(inp["tanfovx"]), float(inp["tanfovy"])
        self.P, self.dev = int(self.means.shape[0]), dev
        self.has_sh, self.has_sr = inp.get("shs") is not None, inp.get("scales") is not None
        out = _C.rasterize_gaussians(self.bg, self.means, self.colors, self.opac, self.scales, self.rots, self.sm, self.cov, self.view, self.proj, self.tfx, self.tfy,
                                     self.H, self.W, self.sh, self.D, self.campos, False, False, **fwd_kw)
        self.R, self.color, self.radii, self.geom, self.binning, self.img = out[:6]

    def alpha(self):
        from diff_gaussian_rasterization import _C
        return _C.alpha_from_state(self.img, self.H, self.W)

    def field(self, name):
        from diff_gaussian_rasterization import _C
        return _C.state_field(name, self.P, self.W, self.H, self.R, self.has_sh, self.has_sr, self.geom, self.binning, self.img)

    def backward(self, dL, g_A=None, **kw):
        from diff_gaussian_rasterization import _C
        if g_A is not None:
            kw["grad_out_alpha"] = _t(g_A, self.dev).reshape(1, self.H, self.W)
        g = _C.rasterize_gaussians_backward(self.bg, self.means, self.radii, self.colors, self.scales, self.rots, self.sm, self.cov, self.view, self.proj, self.tfx,
                                            self.tfy, _t(dL, self.dev), self.sh, self.D, self.campos, self.geom, self.R, self.binning, self.img, False, _with_conic=True, **kw)
        return {n: v.cpu().numpy() for n, v in zip(NAMES, g)}


# ---- forward ----
@pytest.mark.parametrize("name", SCENES)
def test_alpha_is_one_minus_final_T(name, gpu_device):
    s = scene(name)
    f = Frame(s["inp"], gpu_device)
    alpha = f.alpha()
    assert alpha.dtype == torch.float32 and tuple(alpha.shape) == (1, s["H"], s["W"])
    a = alpha.cpu().numpy()[0]
    mine_T = f.field("final_T").cpu().numpy().reshape(s["H"], s["W"])
    assert np.array_equal(a, np.float32(1.0) - mine_T), "alpha is not 1 - final_T of the same frame, bit for bit"
    e = util.rel_l2(a, np.float32(1.0) - s["final_T"])
    print(f"{name}: alpha against 1 - the oracle's final_T: rel-L2 {e:.3e}")
    assert e <= util.tolerance("color", None)
    # exactly 0 on every pixel of a tile without instances
    rg = f.field("ranges").cpu().numpy().reshape(-1, 2)
    gx = (s["W"] + 15) // 16
    empty = 0
    for t in np.nonzero(rg[:, 1] == rg[:, 0])[0]:
        ty, tx = divmod(int(t), gx)
        assert np.all(a[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 0), f"tile {t} has no instance but alpha != 0"
        empty += 1
    if name == "g10_all_culled":
        assert f.R == 0 and empty == len(rg) and np.all(a == 0)
    if name == "cloud_600_sparse":
        assert empty > 0
    # the same bits whatever forward wrote the state: light groups on / off, the speculative forward
    for kw in (dict(light_tiles=True), dict(light_tiles=False), dict(r_guess=max(int(f.R), 1) + 1000), dict(r_guess=max(int(f.R), 1) + 1000, light_tiles=True)):
        assert np.array_equal(Frame(s["inp"], gpu_device, **kw).alpha().cpu().numpy()[0], a), kw


def _rasterizer(inp, dev, bg=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=int(inp["image_height"]), image_width=int(inp["image_width"]), tanfovx=float(inp["tanfovx"]),
                                       tanfovy=float(inp["tanfovy"]), bg=_t(inp["bg"] if bg is None else bg, dev), scale_modifier=float(inp.get("scale_modifier", 1.0)),
                                       viewmatrix=_t(inp["viewmatrix"], dev), projmatrix=_t(inp["projmatrix"], dev), sh_degree=int(inp["sh_degree"]),
                                       campos=_t(inp["campos"], dev), prefiltered=False, debug=False)
    return GaussianRasterizer(rs)


LEAVES = {"means3D": "dL_dmeans3D", "means2D": "dL_dmeans2D", "opacities": "dL_dopacity", "scales": "dL_dscales", "rotations": "dL_drotations", "shs": "dL_dsh"}


def _leaves(inp, dev):
    L = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    L["means2D"] = torch.zeros(inp["means3D"].shape[0], 3, device=dev, requires_grad=True)
    return L


def _render(inp, dev, L, **kw):
    return _rasterizer(inp, dev, kw.pop("bg", None))(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], shs=L["shs"], scales=L["scales"],
                                                      rotations=L["rotations"], **kw)


def test_alpha_of_an_empty_model_and_the_speculative_public_forward(gpu_device, monkeypatch):
    inp = scene("cloud_600_sparse")["inp"]
    empty = dict(inp, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32), shs=np.zeros((0, 4, 3), np.float32))
    color, radii, alpha = _render(empty, gpu_device, _leaves(empty, gpu_device), return_alpha=True)
    assert tuple(alpha.shape) == (1, 40, 72) and alpha.dtype == torch.float32 and bool((alpha == 0).all()) and radii.numel() == 0
    # through the public forward, plain and speculative (the second and third call of a key speculate): the same bits
    import youreditableavatar_amd.diff_gaussian_rasterization as dgr
    with torch.no_grad():
        first = [_render(inp, gpu_device, _leaves(inp, gpu_device), return_alpha=True)[2].cpu().numpy() for _ in range(3)]
        monkeypatch.setattr(dgr, "_SPECULATE", False)
        plain = _render(inp, gpu_device, _leaves(inp, gpu_device), return_alpha=True)[2].cpu().numpy()
    for a in first:
        assert np.array_equal(a, plain)
    assert np.array_equal(plain[0], Frame(inp, gpu_device).alpha().cpu().numpy()[0])


def test_compositing_identity_over_two_backgrounds(gpu_device):
    """alpha does not depend on the background, and colour - (1 - alpha) bg is the same premultiplied colour over both: the frame stores
    fl(C + T bg) (one or two fp32 roundings of a value below 4: <= 2.4e-7 each) and alpha = fl(1 - T) (<= 3e-8); the test itself subtracts
    in double, so the two sides differ by <= 1e-6."""
    s = scene("cloud_6000_classes")
    out = []
    for bg in ((1.0, 1.0, 1.0), (0.1, 0.7, 0.3)):
        f = Frame(dict(s["inp"], bg=np.asarray(bg, np.float32)), gpu_device)
        out.append((f.color.cpu().numpy().astype(np.float64), f.alpha().cpu().numpy(), np.asarray(bg, np.float64).reshape(3, 1, 1)))
    (c1, a1, b1), (c2, a2, b2) = out
    assert np.array_equal(a1, a2) and a1.max() > 0.5 and np.abs(c1).max() < 4.0
    pre1, pre2 = c1 - (1.0 - a1.astype(np.float64)) * b1, c2 - (1.0 - a2.astype(np.float64)) * b2
    d = float(np.abs(pre1 - pre2).max())
    print(f"premultiplied colour over two backgrounds: max abs difference {d:.3e}")
    assert d <= 1e-6


# ---- gradients through the _C surface ----
MODES = {"default": (dict(), dict()), "deterministic": (dict(), dict(deterministic=True)),
         "light_fwd_only": (dict(light_tiles=True), dict(light_tiles=False)), "light_bwd_only": (dict(light_tiles=False), dict(light_tiles=True))}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SCENES)
def test_gradients_with_alpha_upstream(name, mode, gpu_device):
    s = scene(name)
    fwd_kw, bwd_kw = MODES[mode]
    f = Frame(s["inp"], gpu_device, **fwd_kw)
    g = f.backward(s["dL"], s["g_A"], **bwd_kw)
    assert np.array_equal(f.radii.cpu().numpy(), s["radii"])
    check_gradients(g, s["exp"], f"{name} [{mode}]")
    assert np.all(g["dL_dmeans2D"][:, 2] == 0)
    vis = s["radii"] > 0
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D"):
        assert np.all(g[k][~vis] == 0), f"{k}: culled Gaussians must have zero gradient"
    if mode == "deterministic":
        again = f.backward(s["dL"], s["g_A"], **bwd_kw)
        for k in NAMES:
            assert np.array_equal(g[k], again[k]), f"{k}: two deterministic backward passes of one frame differ"


def test_backward_without_the_keyword_is_the_parent_call(gpu_device):
    """grad_out_alpha=None is today's call; a zero alpha gradient through the new kernels gives the same bits in deterministic mode (x - 0 = x)."""
    s = scene("g13_dense_2k")
    f = Frame(s["inp"], gpu_device)
    a, b = f.backward(s["dL"], None, deterministic=True), f.backward(s["dL"], np.zeros_like(s["g_A"]), deterministic=True)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(RuntimeError, match="grad_out_alpha"):
        f.backward(s["dL"], None, grad_out_alpha=torch.zeros(1, 3, 3, device=gpu_device))


# ---- the public API ----
@pytest.fixture
def deterministic_default():
    from diff_gaussian_rasterization import _C
    _C.set_deterministic(True)
    yield
    _C._lib.tgs_set_deterministic(-1)


def _grads(L):
    return {k: (L[k].grad.detach().cpu().numpy() if L[k].grad is not None else None) for k in LEAVES}


def test_return_alpha_false_is_the_two_tuple_of_today(gpu_device, deterministic_default):
    s = scene("cloud_600_sparse")
    inp, dev = s["inp"], gpu_device
    w = _t(s["dL"], dev)
    L0 = _leaves(inp, dev)
    out = _render(inp, dev, L0)
    assert isinstance(out, tuple) and len(out) == 2 and type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBackward")
    (w * out[0]).sum().backward()
    f = Frame(inp, dev)
    direct = f.backward(s["dL"], None, deterministic=True)
    assert np.array_equal(out[0].detach().cpu().numpy(), f.color.cpu().numpy())
    g0 = _grads(L0)
    for leaf, k in LEAVES.items():
        assert np.array_equal(g0[leaf], direct[k].reshape(g0[leaf].shape)), leaf
    # colour alone with return_alpha=True (alpha unused: no alpha gradient reaches the node): bit-identical to return_alpha=False
    L1 = _leaves(inp, dev)
    color, radii, alpha = _render(inp, dev, L1, return_alpha=True)
    assert alpha.requires_grad and not radii.requires_grad
    (w * color).sum().backward()
    g1 = _grads(L1)
    for leaf in LEAVES:
        assert np.array_equal(g0[leaf], g1[leaf]), leaf


def test_alpha_alone_and_both_terms_through_autograd(gpu_device):
    s = scene("cloud_600_sparse")
    inp, dev = s["inp"], gpu_device
    wA, wC = _t(s["g_A"], dev).reshape(1, s["H"], s["W"]), _t(s["dL"], dev)
    # alpha alone: the image is unused, the colour gradient is absent -> the zero-colour oracle run alone
    L = _leaves(inp, dev)
    color, radii, alpha = _render(inp, dev, L, return_alpha=True)
    (wA * alpha).sum().backward()
    g = _grads(L)
    check_gradients({LEAVES[k]: v for k, v in g.items() if k != "shs"}, s["alpha_only"], "alpha alone", keys=SUMMED)
    assert not np.any(g["shs"]), "alpha does not depend on the colours"
    # both terms in one loss: the summed expectation
    L = _leaves(inp, dev)
    color, radii, alpha = _render(inp, dev, L, return_alpha=True)
    ((wC * color).sum() + (wA * alpha).sum()).backward()
    check_gradients({LEAVES[k]: v for k, v in _grads(L).items()}, s["exp"], "colour + alpha")


# ---- the per-pixel half alone, then the batch per-Gaussian pass ----
def test_render_alpha_then_batch_backward_on_one_view(gpu_device):
    """tgs_backward_render_alpha_opt + tgs_backward_batch on one view against tgs_backward_alpha_opt, deterministic.  dL_dmeans2D is the
    same bits (both sum the same tile partials in the same order); the parameter gradients of the batch kernels differ from the per-view
    kernel's in rounding today (tests/test_gpu_batch_backward.py holds them to 2e-5), so they are held to the bar against the expectation
    and their distance from the per-view pass is printed."""
    from diff_gaussian_rasterization import _C
    s = scene("cloud_6000_classes")
    inp, dev = s["inp"], gpu_device
    f = Frame(inp, dev)
    one = f.backward(s["dL"], s["g_A"], deterministic=True)
    _C.rasterize_gaussians_backward_render(f.bg, _t(s["dL"], dev), f.R, f.binning, f.img, f.P, deterministic=True, grad_out_alpha=_t(s["g_A"], dev).reshape(1, s["H"], s["W"]))
    P, M = f.P, int(f.sh.shape[1])
    into = dict(means3D=torch.full((P, 3), float("nan"), device=dev), opacities=torch.full((P, 1), float("nan"), device=dev),
                sh=torch.full((P, M, 3), float("nan"), device=dev), scales=torch.full((P, 3), float("nan"), device=dev), rotations=torch.full((P, 4), float("nan"), device=dev))
    view = dict(viewmatrix=f.view, projmatrix=f.proj, campos=f.campos, tanfovx=f.tfx, tanfovy=f.tfy, image_height=f.H, image_width=f.W, radii=f.radii,
                geom=f.geom, binning=f.binning, img=f.img, R=f.R)
    (g2d, _), = _C.rasterize_gaussians_backward_batch([view], f.means, f.sh, f.D, f.scales, f.rots, f.sm, None, into, accumulate=False)
    assert np.array_equal(g2d.cpu().numpy(), one["dL_dmeans2D"])
    got = {"dL_dmeans2D": g2d.cpu().numpy(), "dL_dmeans3D": into["means3D"].cpu().numpy(), "dL_dopacity": into["opacities"].cpu().numpy(),
           "dL_dsh": into["sh"].cpu().numpy(), "dL_dscales": into["scales"].cpu().numpy(), "dL_drotations": into["rotations"].cpu().numpy()}
    check_gradients(got, s["exp"], "render_alpha + batch")
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh"):
        e = util.rel_l2(got[k], one[k].reshape(got[k].shape))
        print(f"batch against the per-view pass, {k}: rel-L2 {e:.3e}")


def test_example_fits_a_silhouette(gpu_device):
    """examples/fit_silhouette.py: l1(colour) + l1(alpha, mask) through return_alpha=True and autograd, Adam on opacities and scales; the loss falls."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fit_silhouette", os.path.join(util.ROOT, "examples", "fit_silhouette.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    vals = mod.run(steps=12, P=1500, W=96, H=64, V=2, log=lines.append)
    print("\n".join(lines))
    assert len(vals) == 13 and all(np.isfinite(vals)) and vals[-1] < vals[0]
    assert lines[0].startswith("step   0") and lines[1].startswith("step  12")
