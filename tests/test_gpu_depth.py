"""The expected-depth output of the rasterizer (depth = sum_i T_i alpha_i z_i over the pairs the colour frame blended) and its gradients,
on the device.

Yardstick (tests/test_depth_abi.py checks it on the CPU): the oracle's frame of the same geometry with colors_precomp = (z, z, z), no SH and
background 0 has channel 0 == depth, z being the oracle's own depths of the colour frame.  For the upstream (dL_dpix, g_D) the expectation is
    oracle(inp, dL_dpix) + oracle(depth-colour inp, (g_D, 0, 0))      for dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcov3D, dL_dscales,
                                                                      dL_drotations, dL_dmeans3D,
    + dL_dz (x) (m[2], m[6], m[10]), dL_dz = dL_dcolors[:, 0] of the depth-colour run, added to dL_dmeans3D,
    oracle(inp, dL_dpix) alone                                        for dL_dsh / dL_dcolors,
and with a gradient on alpha as well the zero-colour term of tests/test_gpu_alpha.py on top.

Bar: the project's frozen one, computed here from the reference alone -- per tensor min(max(1e-4, 2 eta), 1e-3) with
eta = rel_l2(that expectation from the fp32 oracle, the same from the fp64 oracle).  No failure budget: every scene, every tensor, against
the fp32 expectation.  Scenes, kernel modes and helpers are those of tests/test_gpu_alpha.py."""
import functools

import numpy as np
import pytest
import torch

from tests import test_gpu_alpha as A
from tests import util
from tests.test_depth_abi import depth_colour_input, depth_upstream, z_row

pytestmark = pytest.mark.gpu

SCENES, MODES, NAMES, SUMMED, COLOUR_ONLY, LEAVES = A.SCENES, A.MODES, A.NAMES, A.SUMMED, A.COLOUR_ONLY, A.LEAVES
check_gradients, _t = A.check_gradients, A._t


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> the alpha suite's scene (inputs, dL, g_A, its alpha term) plus g_D, the yardstick's depth and, per oracle build, the colour term and
    the depth term of the expectation (computed once per scene, read-only)"""
    a = A.scene(name)
    inp, H, W = a["inp"], a["H"], a["W"]
    g_D = (np.random.Generator(np.random.PCG64(4048)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    row = z_row(inp["viewmatrix"])
    colour, depth_term, depth, zs = {}, {}, None, None
    for variant in ("f32", "f64"):
        c = util.oracle_run(inp, a["dL"], variant=variant)
        z = np.asarray(c["depths"])
        d = util.oracle_run(depth_colour_input(inp, z), depth_upstream(g_D), variant=variant)
        assert np.array_equal(np.asarray(d["n_contrib"]), np.asarray(c["n_contrib"])), "the depth-colour frame blends other pairs than the colour frame"
        colour[variant] = {k: np.asarray(c[k], np.float64) for k in SUMMED + COLOUR_ONLY}
        t = {k: np.asarray(d[k], np.float64) for k in SUMMED}
        dz = np.asarray(d["dL_dcolors"], np.float64).reshape(-1, 3)[:, 0]
        t["dL_dmeans3D"] = t["dL_dmeans3D"] + (dz[:, None] * row[None, :]).reshape(t["dL_dmeans3D"].shape)
        depth_term[variant] = t
        if variant == "f32":
            depth, zs = np.asarray(d["color"], np.float32)[0], np.asarray(z, np.float32).reshape(-1)
    return dict(a, g_D=g_D, colour=colour, depth_term=depth_term, depth=depth, z=zs)


def expectation(s, colour: bool, alpha: bool) -> dict:
    """the depth term, plus the colour term and the alpha term on request -- for both oracle builds"""
    exp = {}
    for variant in ("f32", "f64"):
        e = {k: s["depth_term"][variant][k].copy() for k in SUMMED}
        e.update({k: np.zeros_like(s["colour"][variant][k]) for k in COLOUR_ONLY})
        if colour:
            for k in SUMMED + COLOUR_ONLY:
                e[k] = e[k] + s["colour"][variant][k]
        if alpha:
            for k in SUMMED:
                e[k] = e[k] + s["alpha_only"][variant][k]
        exp[variant] = e
    return exp


class Frame(A.Frame):
    def depth(self):
        from diff_gaussian_rasterization import _C
        return _C.depth_from_state(self.geom, self.binning, self.img, self.P, self.H, self.W, int(self.R))

    def backward(self, dL, g_A=None, g_D=None, **kw):
        if g_D is not None:
            kw["grad_out_depth"] = _t(g_D, self.dev).reshape(1, self.H, self.W)
        return super().backward(dL, g_A, **kw)


# ---- forward ----
@pytest.mark.parametrize("name", SCENES)
def test_depth_is_the_expected_depth_of_the_colour_frame(name, gpu_device):
    s = scene(name)
    H, W = s["H"], s["W"]
    f = Frame(s["inp"], gpu_device)
    depth = f.depth()
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (1, H, W)
    d = depth.cpu().numpy()[0]
    e = util.rel_l2(d, s["depth"])
    print(f"{name}: depth against channel 0 of the oracle's depth-colour frame: rel-L2 {e:.3e}")
    assert e <= util.tolerance("color", None)
    assert np.array_equal(f.depth().cpu().numpy()[0], d), "two runs over one frame's state differ"
    # exactly 0 on every pixel of a tile without instances
    rg = f.field("ranges").cpu().numpy().reshape(-1, 2) if f.P else np.zeros((0, 2))
    gx = (W + 15) // 16
    empty = 0
    for t in np.nonzero(rg[:, 1] == rg[:, 0])[0]:
        ty, tx = divmod(int(t), gx)
        assert np.all(d[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 0), f"tile {t} has no instance but depth != 0"
        empty += 1
    if name == "g10_all_culled":
        assert f.R == 0 and np.all(d == 0)
    if name == "cloud_600_sparse":
        assert empty > 0
    # the same pairs as alpha = sum T_i alpha_i: alpha min z <= depth <= alpha max z over the visible splats.  Slack: alpha is fl(1 - T_final),
    # depth an fp32 sum of n_contrib products -- each of the n + 2 roundings at most 2^-24 of a partial sum <= max z, doubled for both sides
    vis = s["radii"] > 0
    if vis.any():
        zmin, zmax = float(s["z"][vis].min()), float(s["z"][vis].max())
        alpha = f.alpha().cpu().numpy()[0].astype(np.float64)
        n = f.field("n_contrib").cpu().numpy().reshape(H, W).astype(np.float64)
        slack = (n + 2.0) * 2.0 ** -23 * zmax
        assert zmin > 0 and np.all(d <= alpha * zmax + slack) and np.all(d >= alpha * zmin - slack)
        assert np.all((d > 0) == (n > 0)), "depth is positive exactly where something was blended"
    # the same bits whatever forward wrote the state: light groups on / off, the speculative forward
    for kw in (dict(light_tiles=True), dict(light_tiles=False), dict(r_guess=max(int(f.R), 1) + 1000), dict(r_guess=max(int(f.R), 1) + 1000, light_tiles=True)):
        assert np.array_equal(Frame(s["inp"], gpu_device, **kw).depth().cpu().numpy()[0], d), kw


def test_depth_of_an_empty_model_and_the_output_order(gpu_device, monkeypatch):
    inp = scene("cloud_600_sparse")["inp"]
    empty = dict(inp, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32), shs=np.zeros((0, 4, 3), np.float32))
    out = A._render(empty, gpu_device, A._leaves(empty, gpu_device), return_depth=True)
    assert len(out) == 3 and tuple(out[2].shape) == (1, 40, 72) and out[2].dtype == torch.float32 and bool((out[2] == 0).all()) and out[1].numel() == 0
    out = A._render(empty, gpu_device, A._leaves(empty, gpu_device), return_alpha=True, return_depth=True)
    assert len(out) == 4 and bool((out[2] == 0).all()) and bool((out[3] == 0).all())
    # (color, radii), then alpha, then depth: each the bits of the _C surface, through the plain and the speculative public forward
    f = Frame(inp, gpu_device)
    alpha, depth = f.alpha().cpu().numpy(), f.depth().cpu().numpy()
    assert alpha.max() <= 1.0 < depth.max()                  # (tells the two apart: the cloud lies deeper than 1)
    import youreditableavatar_amd.diff_gaussian_rasterization as dgr
    with torch.no_grad():
        for _ in range(3):                                   # (the second and third call of a key speculate)
            color, radii, a, d = A._render(inp, gpu_device, A._leaves(inp, gpu_device), return_alpha=True, return_depth=True)
            assert np.array_equal(a.cpu().numpy(), alpha) and np.array_equal(d.cpu().numpy(), depth)
        monkeypatch.setattr(dgr, "_SPECULATE", False)
        color, radii, d = A._render(inp, gpu_device, A._leaves(inp, gpu_device), return_depth=True)
        assert np.array_equal(d.cpu().numpy(), depth) and np.array_equal(color.cpu().numpy(), f.color.cpu().numpy())


# ---- gradients through the _C surface ----
UPSTREAMS = {"depth alone": (False, False), "colour + depth": (True, False), "colour + alpha + depth": (True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SCENES)
def test_gradients_with_depth_upstream(name, mode, gpu_device):
    s = scene(name)
    fwd_kw, bwd_kw = MODES[mode]
    f = Frame(s["inp"], gpu_device, **fwd_kw)
    assert np.array_equal(f.radii.cpu().numpy(), s["radii"])
    vis = s["radii"] > 0
    for what, (colour, alpha) in UPSTREAMS.items():
        dL = s["dL"] if colour else np.zeros_like(s["dL"])
        g = f.backward(dL, s["g_A"] if alpha else None, s["g_D"], **bwd_kw)
        check_gradients(g, expectation(s, colour, alpha), f"{name} [{mode}] {what}")
        assert np.all(g["dL_dmeans2D"][:, 2] == 0)
        for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D"):
            assert np.all(g[k][~vis] == 0), f"{k}: culled Gaussians must have zero gradient"
        if not colour:
            assert not np.any(g["dL_dsh"]) and not np.any(g["dL_dcolors"]), "depth does not depend on the colours"
        if mode == "deterministic":
            again = f.backward(dL, s["g_A"] if alpha else None, s["g_D"], **bwd_kw)
            for k in NAMES:
                assert np.array_equal(g[k], again[k]), f"{k}: two deterministic backward passes of one frame differ"


def test_backward_without_the_keyword_is_the_alpha_call(gpu_device):
    """grad_out_depth=None launches no depth kernel: the bits of the call without the keyword, with and without an alpha gradient; a zero
    depth gradient through the depth kernels adds zeros (x + 0 = x; the conic shares are split into hi + lo again, which keeps hi + lo's
    double value, so dL_dconic and what follows from it are held to equality through the deterministic per-pixel kernel as well)."""
    s = scene("g13_dense_2k")
    f = Frame(s["inp"], gpu_device)
    for g_A in (None, s["g_A"]):
        a, b = f.backward(s["dL"], g_A, deterministic=True), f.backward(s["dL"], g_A, None, deterministic=True)
        z = f.backward(s["dL"], g_A, np.zeros_like(s["g_D"]), deterministic=True)
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), k
            assert np.array_equal(a[k], z[k]), k
    with pytest.raises(RuntimeError, match="grad_out_depth"):
        f.backward(s["dL"], None, grad_out_depth=torch.zeros(1, 3, 3, device=gpu_device))


# ---- the public API ----
def _grads(L):
    return A._grads(L)


def test_return_depth_false_is_the_two_tuple_and_an_unused_depth_changes_nothing(gpu_device, deterministic_default):
    s = scene("cloud_600_sparse")
    inp, dev = s["inp"], gpu_device
    w = _t(s["dL"], dev)
    L0 = A._leaves(inp, dev)
    out = A._render(inp, dev, L0, return_depth=False)
    assert isinstance(out, tuple) and len(out) == 2 and type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBackward")
    (w * out[0]).sum().backward()
    g0 = _grads(L0)
    # colour alone with return_depth=True (depth unused: no depth gradient reaches the node): bit-identical to the plain node
    for kw in (dict(return_depth=True), dict(return_alpha=True, return_depth=True)):
        L1 = A._leaves(inp, dev)
        res = A._render(inp, dev, L1, **kw)
        assert len(res) == 2 + len(kw) and res[-1].requires_grad and not res[1].requires_grad
        (w * res[0]).sum().backward()
        g1 = _grads(L1)
        for leaf in LEAVES:
            assert np.array_equal(g0[leaf], g1[leaf]), (leaf, kw)


deterministic_default = A.deterministic_default


def test_depth_terms_through_autograd(gpu_device):
    s = scene("cloud_600_sparse")
    inp, dev = s["inp"], gpu_device
    wD, wA, wC = _t(s["g_D"], dev).reshape(1, s["H"], s["W"]), _t(s["g_A"], dev).reshape(1, s["H"], s["W"]), _t(s["dL"], dev)
    as_exp = lambda L: {LEAVES[k]: v for k, v in _grads(L).items()}
    # depth alone: the image is unused, the colour gradient is absent
    L = A._leaves(inp, dev)
    color, radii, depth = A._render(inp, dev, L, return_depth=True)
    (wD * depth).sum().backward()
    g = as_exp(L)
    assert not np.any(g.pop("dL_dsh")), "depth does not depend on the colours"
    check_gradients(g, expectation(s, False, False), "depth alone", keys=SUMMED)
    # colour + depth in one loss
    L = A._leaves(inp, dev)
    color, radii, depth = A._render(inp, dev, L, return_depth=True)
    ((wC * color).sum() + (wD * depth).sum()).backward()
    check_gradients(as_exp(L), expectation(s, True, False), "colour + depth")
    # colour + alpha + depth
    L = A._leaves(inp, dev)
    color, radii, alpha, depth = A._render(inp, dev, L, return_alpha=True, return_depth=True)
    ((wC * color).sum() + (wA * alpha).sum() + (wD * depth).sum()).backward()
    check_gradients(as_exp(L), expectation(s, True, True), "colour + alpha + depth")
    # alpha used, depth returned and unused: the alpha suite's expectation
    L = A._leaves(inp, dev)
    color, radii, alpha, depth = A._render(inp, dev, L, return_alpha=True, return_depth=True)
    ((wC * color).sum() + (wA * alpha).sum()).backward()
    check_gradients(as_exp(L), s["exp"], "colour + alpha, depth unused")


def test_example_fits_a_depth_map(gpu_device):
    """examples/fit_depth.py: l1(depth / alpha, target) through return_alpha=True, return_depth=True and autograd, Adam on positions and
    opacities; the loss falls."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fit_depth", os.path.join(util.ROOT, "examples", "fit_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    vals = mod.run(steps=12, P=1500, W=96, H=64, log=lines.append)
    print("\n".join(lines))
    assert len(vals) == 13 and all(np.isfinite(vals)) and vals[-1] < vals[0]
