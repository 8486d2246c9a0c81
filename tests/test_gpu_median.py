"""The median-depth and surface-index outputs of the rasterizer (z and Gaussian index of the first blended pair after which the
transmittance falls below one half) and the median's gradient, on the device.

Yardstick (tests/test_median_abi.py computes and checks it on the CPU): a NumPy walk of the oracle's own lists that restates the
definition, in float32 on the fp32 oracle's state and in float64 on the fp64 oracle's.  Index and depth are compared on the pixels that
are not AMBIGUOUS there (the two walks disagree, or a blended pair leaves T within 0.5e-4 of one half); by Gaussian index, never by list
position -- with instance pruning the device's lists are shorter than the oracle's.

Gradient: median_depth is piecewise constant in every alpha, so under an upstream g_M (zeroed on the ambiguous pixels: the expectation
then comes from the reference alone)
    dz[i] = sum over the pixels whose median entry is i of g_M           (float64, from the yardstick's index map)
    dL_dmeans3D = the oracle's colour term + dz (x) (m[2], m[6], m[10])
and every other gradient is the colour term alone.  Bar: the frozen one of the alpha and depth suites (check_gradients:
min(max(1e-4, 2 eta), 1e-3) per tensor, eta from the fp32 and fp64 expectations), no failure budget.  Scenes, kernel modes and helpers
are those of tests/test_gpu_alpha.py / tests/test_gpu_depth.py."""
import functools

import numpy as np
import pytest
import torch

from tests import test_gpu_alpha as A
from tests import test_gpu_depth as D
from tests import test_gpu_features as Fe
from tests import util
from tests.test_depth_abi import z_row
from tests.test_features_abi import make_features
from tests.test_median_abi import yardstick

pytestmark = pytest.mark.gpu

SCENES, MODES, NAMES, SUMMED, COLOUR_ONLY, LEAVES = A.SCENES, A.MODES, A.NAMES, A.SUMMED, A.COLOUR_ONLY, A.LEAVES
check_gradients, _t = A.check_gradients, A._t
deterministic_default = A.deterministic_default
FORWARDS = (dict(light_tiles=True), dict(light_tiles=False), "r_guess", "r_guess+light")      # the keyword sets of the depth suite's forward test


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> the depth suite's scene (inputs, dL, g_A, g_D, colour / alpha / depth terms per oracle build) plus the yardstick, g_M (zero on the
    ambiguous pixels) and the median's share of dL_dmeans3D in float64 (computed once per scene, read-only)"""
    d, y = D.scene(name), yardstick(name)
    H, W = d["H"], d["W"]
    g_M = (np.random.Generator(np.random.PCG64(5051)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    g_M[y["ambiguous"]] = 0.0
    idx = y["f32"]["index"]
    P = int(np.asarray(d["inp"]["means3D"]).shape[0])
    dz = np.zeros(P, np.float64)
    np.add.at(dz, idx[idx >= 0], g_M[idx >= 0].astype(np.float64))
    share = dz[:, None] * z_row(d["inp"]["viewmatrix"])[None, :]
    return dict(d, y=y, g_M=g_M, dz=dz, share=share, ok=~y["ambiguous"], index=idx)


def expectation(s, colour: bool, alpha: bool, depth: bool) -> dict:
    """the median's share on dL_dmeans3D, plus the colour / alpha / depth terms on request -- for both oracle builds"""
    exp = {}
    for variant in ("f32", "f64"):
        e = {k: np.zeros_like(s["colour"][variant][k]) for k in SUMMED + COLOUR_ONLY}
        if colour:
            for k in SUMMED + COLOUR_ONLY:
                e[k] = e[k] + s["colour"][variant][k]
        if alpha:
            for k in SUMMED:
                e[k] = e[k] + s["alpha_only"][variant][k]
        if depth:
            for k in SUMMED:
                e[k] = e[k] + s["depth_term"][variant][k]
        e["dL_dmeans3D"] = e["dL_dmeans3D"] + s["share"].reshape(e["dL_dmeans3D"].shape)
        exp[variant] = e
    return exp


class Frame(D.Frame):
    def median(self):
        from diff_gaussian_rasterization import _C
        return _C.median_from_state(self.geom, self.binning, self.img, self.P, self.H, self.W, int(self.R))

    def backward(self, dL, g_A=None, g_D=None, g_M=None, pos=None, **kw):
        if g_M is not None:
            kw["grad_out_median"], kw["median_pos"] = _t(g_M, self.dev).reshape(1, self.H, self.W), pos
        return super().backward(dL, g_A, g_D, **kw)


def _fwd_kw(kw, f):
    if kw == "r_guess":
        return dict(r_guess=max(int(f.R), 1) + 1000)
    if kw == "r_guess+light":
        return dict(r_guess=max(int(f.R), 1) + 1000, light_tiles=True)
    return kw


# ---- forward ----
@pytest.mark.parametrize("name", SCENES)
def test_median_is_the_first_entry_behind_which_T_falls_below_one_half(name, gpu_device):
    s = scene(name)
    H, W, ok = s["H"], s["W"], s["ok"]
    f = Frame(s["inp"], gpu_device)
    md, mi, mp = f.median()
    assert md.dtype == torch.float32 and mi.dtype == torch.int32 and mp.dtype == torch.int32
    assert tuple(md.shape) == tuple(mi.shape) == tuple(mp.shape) == (1, H, W)
    d, i, p = md.cpu().numpy()[0], mi.cpu().numpy()[0], mp.cpu().numpy()[0]
    # the index: the yardstick's on every unambiguous pixel, exactly
    wrong = int((i[ok] != s["index"][ok]).sum())
    print(f"{name}: {int(ok.sum())} unambiguous pixels of {H * W}, {int((i >= 0).sum())} with a median entry, {wrong} indices differ from the yardstick")
    assert wrong == 0
    assert i.min() >= -1 and i.max() < max(f.P, 1)
    has = i >= 0
    assert np.all(d[~has] == 0) and np.array_equal(p > 0, has) and np.all(p[~has] == 0)
    if f.P and f.R:
        # the depth: the device's own depth of that Gaussian, bit for bit; against the oracle's within the colour tolerance
        z = f.field("depths").cpu().numpy()
        assert np.array_equal(d[has], z[i[has]]), "median_depth is not the frame's own z of median_index"
        sel = ok & has
        e = util.rel_l2(d[sel], s["y"]["depths_f32"][s["index"][sel]])
        print(f"{name}: median depth against the oracle's depths[index]: rel-L2 {e:.3e}")
        assert e <= util.tolerance("color", None)
        # a median entry exactly where the frame's own final T is below one half
        fT = f.field("final_T").cpu().numpy().reshape(H, W)
        assert np.array_equal(has[ok], (fT < np.float32(0.5))[ok])
        # median_pos names the entry: 1-based position in the tile's list
        rg = f.field("ranges").cpu().numpy().reshape(-1, 2).astype(np.int64)
        pl = f.field("point_list").cpu().numpy().astype(np.int64)
        gx = (W + 15) // 16
        ys, xs = np.nonzero(has)
        tiles = (ys // 16) * gx + xs // 16
        at = rg[tiles, 0] + p[ys, xs] - 1
        assert np.all(at < rg[tiles, 1]) and np.array_equal(pl[at], i[ys, xs])
        # -1 / 0 exactly on every pixel of a tile without instances
        empty = 0
        for t in np.nonzero(rg[:, 1] == rg[:, 0])[0]:
            ty, tx = divmod(int(t), gx)
            blk = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
            assert np.all(i[blk] == -1) and np.all(d[blk] == 0) and np.all(p[blk] == 0), f"tile {t} has no instance but a median entry"
            empty += 1
        if name == "cloud_600_sparse":
            assert empty > 0
    if name == "g10_all_culled":
        assert f.R == 0 and np.all(i == -1) and np.all(d == 0) and np.all(p == 0)
    else:
        assert has.any()


@pytest.mark.parametrize("name", SCENES)
def test_same_bits_from_two_runs_and_whichever_forward_wrote_the_state(name, gpu_device):
    s = scene(name)
    f = Frame(s["inp"], gpu_device)
    first = [x.cpu().numpy() for x in f.median()]
    for a, b in zip(first, f.median()):
        assert np.array_equal(a, b.cpu().numpy()), "two runs over one frame's state differ"
    for kw in FORWARDS:
        kw = _fwd_kw(kw, f)
        for a, b in zip(first[:2], Frame(s["inp"], gpu_device, **kw).median()[:2]):        # (depth and index; positions are a frame's own)
            assert np.array_equal(a, b.cpu().numpy()), kw


# ---- gradients through the _C surface ----
UPSTREAMS = {"colour + median": (True, False, False), "colour + alpha + median": (True, True, False), "colour + alpha + depth + median": (True, True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SCENES)
def test_gradients_with_median_upstream(name, mode, gpu_device):
    s = scene(name)
    fwd_kw, bwd_kw = MODES[mode]
    f = Frame(s["inp"], gpu_device, **fwd_kw)
    assert np.array_equal(f.radii.cpu().numpy(), s["radii"])
    pos = f.median()[2]
    vis = s["radii"] > 0
    row = z_row(s["inp"]["viewmatrix"])
    # a zero colour gradient: the median's share alone
    g = f.backward(np.zeros_like(s["dL"]), None, None, s["g_M"], pos, **bwd_kw)
    e = util.rel_l2(g["dL_dmeans3D"], s["share"])
    print(f"{name} [{mode}] median alone dL_dmeans3D against dz (x) z_row: rel-L2 {e:.3e}")
    if np.any(s["share"]):
        assert e <= 1e-6
    else:
        assert not np.any(g["dL_dmeans3D"])
    for k in NAMES:
        if k != "dL_dmeans3D":
            assert not np.any(g[k]), f"{k}: the median depth reaches the positions alone"
    assert not np.any(g["dL_dmeans3D"][~vis]), "culled Gaussians must have zero gradient"
    # dz itself, along the z row (the row's largest component)
    c = int(np.argmax(np.abs(row)))
    if np.any(s["dz"]):
        assert util.rel_l2(g["dL_dmeans3D"][:, c] / row[c], s["dz"]) <= 1e-6
    # with the colour's, the alpha's and the depth's upstream gradients: the shares add up
    for what, (colour, alpha, depth) in UPSTREAMS.items():
        g = f.backward(s["dL"], s["g_A"] if alpha else None, s["g_D"] if depth else None, s["g_M"], pos, **bwd_kw)
        check_gradients(g, expectation(s, colour, alpha, depth), f"{name} [{mode}] {what}")
        assert np.all(g["dL_dmeans2D"][:, 2] == 0)
        for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D"):
            assert np.all(g[k][~vis] == 0), f"{k}: culled Gaussians must have zero gradient"
        if mode == "deterministic":
            again = f.backward(s["dL"], s["g_A"] if alpha else None, s["g_D"] if depth else None, s["g_M"], pos, **bwd_kw)
            for k in NAMES:
                assert np.array_equal(g[k], again[k]), f"{k}: two deterministic backward passes of one frame differ"


def test_backward_without_the_keyword_is_todays_call_and_the_accumulating_call_adds_the_share(gpu_device):
    from diff_gaussian_rasterization import _C
    s = scene("g13_dense_2k")
    f = Frame(s["inp"], gpu_device)
    pos = f.median()[2]
    a, b = f.backward(s["dL"], deterministic=True), f.backward(s["dL"], None, None, None, None, deterministic=True)
    z = f.backward(s["dL"], None, None, np.zeros_like(s["g_M"]), pos, deterministic=True)
    m = f.backward(s["dL"], None, None, s["g_M"], pos, deterministic=True)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
        if k != "dL_dmeans3D":
            assert np.array_equal(a[k], m[k]), f"{k}: the median depth reaches the positions alone"
    assert util.rel_l2(z["dL_dmeans3D"], a["dL_dmeans3D"]) == 0.0            # (x + 0 = x)
    assert not np.array_equal(a["dL_dmeans3D"], m["dL_dmeans3D"])
    with pytest.raises(RuntimeError, match="grad_out_median"):
        f.backward(s["dL"], grad_out_median=torch.zeros(1, 3, 3, device=gpu_device), median_pos=pos)
    with pytest.raises(RuntimeError, match="median_pos"):
        f.backward(s["dL"], grad_out_median=_t(s["g_M"], gpu_device).reshape(1, s["H"], s["W"]))
    # the accumulating call: into["means3D"] += what the storing call returns
    P, M = f.P, int(f.sh.shape[1])
    into = dict(means3D=torch.zeros((P, 3), device=gpu_device), opacities=torch.zeros((P, 1), device=gpu_device), sh=torch.zeros((P, M, 3), device=gpu_device),
                scales=torch.zeros((P, 3), device=gpu_device), rotations=torch.zeros((P, 4), device=gpu_device))
    args = (f.bg, f.means, f.radii, f.colors, f.scales, f.rots, f.sm, f.cov, f.view, f.proj, f.tfx, f.tfy, _t(s["dL"], gpu_device), f.sh, f.D, f.campos, f.geom, f.R, f.binning,
            f.img, False, into)
    _C.rasterize_gaussians_backward_accumulate(*args, deterministic=True, grad_out_median=_t(s["g_M"], gpu_device).reshape(1, s["H"], s["W"]), median_pos=pos)
    assert np.array_equal(into["means3D"].cpu().numpy(), m["dL_dmeans3D"])
    assert np.array_equal(into["opacities"].cpu().numpy(), m["dL_dopacity"])
    # ... and so for every gradient, with every upstream in one call, on both kinds of model
    for name in ("cloud_600_sparse", "g05_precomp_cov3d"):
        _stored_against_accumulated(name, gpu_device)


INTO = {"means3D": "dL_dmeans3D", "opacities": "dL_dopacity", "sh": "dL_dsh", "colors_precomp": "dL_dcolors", "scales": "dL_dscales", "rotations": "dL_drotations",
        "cov3D_precomp": "dL_dcov3D", "features": "dL_dfeatures"}          # key of ``into`` -> the storing call's name for that gradient
F_NAMES = NAMES[:8] + ("dL_dfeatures",)                   # the storing call's tuple without _with_conic, with a feature gradient
C_ALL = 3


def _all_upstreams(name, dev):
    """-> the scene, a frame of it, the accumulating call's positional arguments without ``into``, and colour + alpha + depth + median +
    features (C = 3) as the keywords of both exports"""
    from diff_gaussian_rasterization import _C
    s = scene(name)
    H, W = s["H"], s["W"]
    f = Fe.Frame(s["inp"], dev)
    pos = _C.median_from_state(f.geom, f.binning, f.img, f.P, H, W, int(f.R))[2]
    g_F = (np.random.Generator(np.random.PCG64(5153)).standard_normal((C_ALL, H, W)) / (H * W)).astype(np.float32)
    maps = {"grad_out_" + k: _t(s[g], dev).reshape(1, H, W) for k, g in (("alpha", "g_A"), ("depth", "g_D"), ("median", "g_M"))}
    kw = dict(maps, median_pos=pos, grad_out_features=_t(g_F, dev), features=_t(make_features(f.P, C_ALL, seed=103), dev))
    args = (f.bg, f.means, f.radii, f.colors, f.scales, f.rots, f.sm, f.cov, f.view, f.proj, f.tfx, f.tfy, _t(s["dL"], dev), f.sh, f.D, f.campos, f.geom, f.R, f.binning,
            f.img, False)
    return s, f, args, kw


def _into(f, fill, dev):
    """every destination the frame's model has, filled with ``fill``"""
    M = int(f.sh.shape[1]) if f.has_sh else 0
    shapes = dict(means3D=(f.P, 3), opacities=(f.P, 1), features=(f.P, C_ALL))
    shapes.update(dict(sh=(f.P, M, 3)) if f.has_sh else dict(colors_precomp=(f.P, 3)))
    shapes.update(dict(scales=(f.P, 3), rotations=(f.P, 4)) if f.has_sr else dict(cov3D_precomp=(f.P, 6)))
    return {k: torch.full(shape, fill, dtype=torch.float32, device=dev) for k, shape in shapes.items()}


def _stored_against_accumulated(name, dev):
    """One implementation under both exports: into zeroed buffers the accumulating call leaves the storing call's bits (0 + x = x), in every
    gradient; into buffers of 0.25 it leaves 0.25 + x -- one fp32 addition per element (relative error <= 2^-24 each), the bar the two
    paths of tests/test_gpu_api.py are held to: rel-L2 <= 1e-6."""
    from diff_gaussian_rasterization import _C
    s, f, args, kw = _all_upstreams(name, dev)
    assert (f.has_sh, f.has_sr) == ((True, True) if name == "cloud_600_sparse" else (False, False)) and f.R > 0
    assert name != "cloud_600_sparse" or (s["W"] % 16 and s["H"] % 16)      # 72 x 40: partial tiles at both edges (the fixture is 48 x 64: whole tiles)
    stored = [dict(zip(F_NAMES, (g.cpu().numpy() for g in _C.rasterize_gaussians_backward(*args, deterministic=True, **kw)))) for _ in range(2)]
    assert len(stored[0]) == 9
    for k in F_NAMES:
        assert np.array_equal(stored[0][k], stored[1][k]), f"{name} {k}: two deterministic storing calls differ"
    assert np.any(stored[0]["dL_dfeatures"]) and np.any(stored[0]["dL_dmeans3D"])
    for run in range(2):
        into = _into(f, 0.0, dev)
        g2d = _C.rasterize_gaussians_backward_accumulate(*args, into, deterministic=True, **kw)
        assert np.array_equal(g2d.cpu().numpy(), stored[0]["dL_dmeans2D"]), f"{name} dL_dmeans2D (run {run})"
        for k, g in into.items():
            assert np.array_equal(g.cpu().numpy(), stored[0][INTO[k]].reshape(g.shape)), f"{name} into[{k}] (run {run}) is not the storing call's {INTO[k]}"
    into = _into(f, 0.25, dev)
    g2d = _C.rasterize_gaussians_backward_accumulate(*args, into, deterministic=True, **kw)
    assert np.array_equal(g2d.cpu().numpy(), stored[0]["dL_dmeans2D"])
    for k, g in into.items():
        e = util.rel_l2(g.cpu().numpy(), 0.25 + stored[0][INTO[k]].reshape(g.shape).astype(np.float64))
        print(f"{name}: into[{k}] = 0.25 + {INTO[k]}: rel-L2 {e:.3e}")
        assert e <= 1e-6, (name, k, e)


def test_both_backward_exports_reject_a_mistake_in_the_same_words_before_any_launch(gpu_device):
    from diff_gaussian_rasterization import _C
    dev = gpu_device
    s, f, args, ok = _all_upstreams("cloud_600_sparse", dev)
    H, W, P = s["H"], s["W"], f.P
    z = lambda *shape, **k: torch.zeros(*shape, device=dev, **k)
    into = _into(f, 0.25, dev)

    def message(fn):
        with pytest.raises(RuntimeError) as e:
            fn()
        return str(e.value)

    feat = dict(grad_out_features=ok["grad_out_features"], features=ok["features"])
    med = dict(grad_out_median=ok["grad_out_median"], median_pos=ok["median_pos"])
    upstream = [("grad_out_alpha", dict(grad_out_alpha=z(1, 3, 3))), ("grad_out_depth", dict(grad_out_depth=z(1, H, W + 1))),
                ("grad_out_features", dict(feat, grad_out_features=z(C_ALL, 3, 3))), ("grad_out_median", dict(med, grad_out_median=z(1, 3, 3))),
                ("features", dict(grad_out_features=ok["grad_out_features"])),
                ("features", dict(grad_out_features=z(0, H, W), features=z(P, 0))), ("features", dict(grad_out_features=z(17, H, W), features=z(P, 17))),
                ("median_pos", dict(grad_out_median=ok["grad_out_median"])), ("median_pos", dict(med, median_pos=ok["median_pos"].float()))]
    for word, kw in upstream:
        a = message(lambda: _C.rasterize_gaussians_backward(*args, **kw))
        b = message(lambda: _C.rasterize_gaussians_backward_accumulate(*args, into, **kw))
        assert a == b and word in a and next(iter(kw)) in a, (kw.keys(), a, b)
    wrong = [("means3D", dict(into, means3D=z(P, 4)), {}), ("means3D", dict(into, means3D=z(P, 3, dtype=torch.float64)), {}),
             ("means3D", dict(into, means3D=z(3, P).t()), {}), ('into["features"]', {k: v for k, v in into.items() if k != "features"}, feat)]
    for word, bad, kw in wrong:
        text = message(lambda: _C.rasterize_gaussians_backward_accumulate(*args, bad, **kw))
        assert word in text and (word != "means3D" or f"[{P}, 3]" in text), text
    torch.cuda.synchronize()
    for k, g in into.items():
        assert bool((g == 0.25).all()), f"a rejected call wrote into[{k}]"


def test_the_accumulating_backward_of_an_empty_model_touches_nothing(gpu_device):
    from diff_gaussian_rasterization import _C
    dev = gpu_device
    inp = scene("cloud_600_sparse")["inp"]
    empty = dict(inp, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32), shs=np.zeros((0, 4, 3), np.float32))
    f = Frame(empty, dev)
    into = {k: torch.full((5, n), 0.25, device=dev) for k, n in (("means3D", 3), ("opacities", 1), ("scales", 3), ("rotations", 4))}
    g2d = _C.rasterize_gaussians_backward_accumulate(f.bg, f.means, f.radii, f.colors, f.scales, f.rots, f.sm, f.cov, f.view, f.proj, f.tfx, f.tfy,
                                                     torch.zeros(3, f.H, f.W, device=dev), f.sh, f.D, f.campos, f.geom, f.R, f.binning, f.img, False, into, deterministic=True)
    assert tuple(g2d.shape) == (0, 3) and g2d.dtype == torch.float32 and g2d.device == f.means.device
    torch.cuda.synchronize()
    assert all(bool((g == 0.25).all()) for g in into.values())


# ---- the public API ----
def _grads(L):
    return A._grads(L)


def test_output_order_for_every_flag_combination_and_the_empty_model(gpu_device):
    s = scene("cloud_600_sparse")
    inp, dev, H, W = s["inp"], gpu_device, s["H"], s["W"]
    f = Frame(inp, dev)
    alpha, depth = f.alpha().cpu().numpy(), f.depth().cpu().numpy()
    md, mi, _ = [x.cpu().numpy() for x in f.median()]
    F = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).standard_normal((f.P, 3)).astype(np.float32)).to(dev)
    with torch.no_grad():
        for ra in (False, True):
            for rd in (False, True):
                for feat in (None, F):
                    kw = dict(return_alpha=ra, return_depth=rd, return_median=True)
                    if feat is not None:
                        kw["features"] = feat
                    out = list(A._render(inp, dev, A._leaves(inp, dev), **kw))
                    assert len(out) == 4 + ra + rd + (feat is not None), kw
                    assert np.array_equal(out.pop(0).cpu().numpy(), f.color.cpu().numpy()) and out.pop(0).dtype == torch.int32
                    if ra:
                        assert np.array_equal(out.pop(0).cpu().numpy(), alpha)
                    if rd:
                        assert np.array_equal(out.pop(0).cpu().numpy(), depth)
                    d, i = out.pop(0), out.pop(0)
                    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (1, H, W)
                    assert np.array_equal(d.cpu().numpy(), md) and np.array_equal(i.cpu().numpy(), mi)
                    if feat is not None:
                        assert tuple(out.pop(0).shape) == (3, H, W)
                    assert not out
    L = A._leaves(inp, dev)
    color, radii, d, i = A._render(inp, dev, L, return_median=True)
    assert d.requires_grad and i.requires_grad is False and radii.requires_grad is False
    # an empty model: zeros and -1, no native median call
    empty = dict(inp, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), scales=np.zeros((0, 3), np.float32),
                 rotations=np.zeros((0, 4), np.float32), shs=np.zeros((0, 4, 3), np.float32))
    L = A._leaves(empty, dev)
    color, radii, d, i = A._render(empty, dev, L, return_median=True)
    assert tuple(d.shape) == tuple(i.shape) == (1, H, W) and bool((d == 0).all()) and bool((i == -1).all()) and i.dtype == torch.int32 and radii.numel() == 0
    (d.sum() + color.sum()).backward()
    assert L["means3D"].grad is None or L["means3D"].grad.numel() == 0


def test_without_the_flag_nothing_changes_and_an_unused_median_launches_no_median_kernel(gpu_device, deterministic_default, monkeypatch):
    from diff_gaussian_rasterization import _C
    s = scene("cloud_600_sparse")
    inp, dev = s["inp"], gpu_device
    w = _t(s["dL"], dev)
    L0 = A._leaves(inp, dev)
    out = A._render(inp, dev, L0, return_median=False)
    again = A._render(inp, dev, A._leaves(inp, dev))
    assert isinstance(out, tuple) and len(out) == 2 and len(again) == 2 and type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBackward")
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])
    (w * out[0]).sum().backward()
    g0 = _grads(L0)
    seen = []
    real = _C.rasterize_gaussians_backward
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", lambda *a, **kw: (seen.append(sorted(kw)), real(*a, **kw))[1])
    for kw in (dict(return_median=True), dict(return_alpha=True, return_depth=True, return_median=True)):
        L1 = A._leaves(inp, dev)
        res = A._render(inp, dev, L1, **kw)
        (w * res[0]).sum().backward()                        # the median depth is returned and unused: no median gradient reaches the node
        assert "grad_out_median" not in seen[-1] and "median_pos" not in seen[-1]
        g1 = _grads(L1)
        for leaf in LEAVES:
            assert np.array_equal(g0[leaf], g1[leaf]), (leaf, kw)


def test_median_terms_through_autograd_equal_the_C_surface(gpu_device, deterministic_default):
    s = scene("cloud_600_sparse")
    inp, dev, H, W = s["inp"], gpu_device, s["H"], s["W"]
    wM, wA, wD = (_t(s[k], dev).reshape(1, H, W) for k in ("g_M", "g_A", "g_D"))
    wC = _t(s["dL"], dev)
    f = Frame(inp, dev)
    pos = f.median()[2]
    as_exp = lambda L: {LEAVES[k]: v for k, v in _grads(L).items()}
    # median alone: the image is unused, the colour gradient is absent
    L = A._leaves(inp, dev)
    color, radii, md, mi = A._render(inp, dev, L, return_median=True)
    (wM * md).sum().backward()
    g = as_exp(L)
    assert util.rel_l2(g["dL_dmeans3D"], s["share"]) <= 1e-6
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh"):
        assert not np.any(g[k]), k
    # colour + median, and all four outputs in one loss: the gradients of the _C surface, bit for bit, and within the bar of the expectation
    L = A._leaves(inp, dev)
    color, radii, md, mi = A._render(inp, dev, L, return_median=True)
    ((wC * color).sum() + (wM * md).sum()).backward()
    g, direct = as_exp(L), f.backward(s["dL"], None, None, s["g_M"], pos, deterministic=True)
    for k in g:
        assert np.array_equal(g[k], direct[k].reshape(g[k].shape)), k
    check_gradients(g, expectation(s, True, False, False), "colour + median through autograd")
    L = A._leaves(inp, dev)
    color, radii, alpha, depth, md, mi = A._render(inp, dev, L, return_alpha=True, return_depth=True, return_median=True)
    ((wC * color).sum() + (wA * alpha).sum() + (wD * depth).sum() + (wM * md).sum()).backward()
    g, direct = as_exp(L), f.backward(s["dL"], s["g_A"], s["g_D"], s["g_M"], pos, deterministic=True)
    for k in g:
        assert np.array_equal(g[k], direct[k].reshape(g[k].shape)), k
    check_gradients(g, expectation(s, True, True, True), "colour + alpha + depth + median through autograd")


def test_example_picks_gaussians_under_a_mask_and_fits_a_median_depth_map(gpu_device):
    """examples/pick_and_fit_median.py: a rectangle mask lifted to Gaussians through median_index, then l1(median_depth, target) through
    return_median=True and autograd, FusedAdam on the positions; the loss falls."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pick_and_fit_median", os.path.join(util.ROOT, "examples", "pick_and_fit_median.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    picked, vals = mod.run(steps=12, P=1500, W=96, H=64, log=lines.append)
    print("\n".join(lines))
    assert picked > 0 and len(vals) == 13 and all(np.isfinite(vals)) and vals[-1] < vals[0]
