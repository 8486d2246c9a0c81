"""Alpha and depth in the whole-batch path: tgs_outputs_views, tgs_backward_render_views_extras_opt, tgs_backward_batch_depth_range
(k_depth_bwd_gauss_views) through the _C bindings, and SyncFreeBatch.run_views(return_alpha=, return_depth=) on every route.

Yardstick: the CPU oracle alone, composed as the one-view suites compose it (tests/test_alpha_abi.py, tests/test_depth_abi.py).  Per view,
for dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dscales, dL_drotations:
    oracle(inp, dL) + oracle(zero-colour inp, (-g_A, 0, 0)) + oracle(depth-colour inp, (g_D, 0, 0)),  + dL_dz (x) (m[2], m[6], m[10]) on dL_dmeans3D;
dL_dsh / dL_dcolors take the colour term alone.  Parameter gradients are summed over the views in float64; dL_dmeans2D (and dL_dcolors on the
colors_precomp path) are compared per view.  Maps: alpha against 1 - final_T, depth against channel 0 of the depth-colour frame, both at
util.tolerance("color", None).

Bar: the frozen one, per tensor min(max(1e-4, 2 eta), 1e-3) with eta = rel_l2(that expectation from the fp32 oracle, from the fp64 oracle),
computed here; the 1e-3 cap is a condition (asserted), no failure budget.  Scenes: tests.test_gpu_batch_backward.make_scene, 176 x 112, unmixed,
scales + rotations; per-view g_A / g_D = standard_normal / (H W) from PCG64(2024 + v) / PCG64(4048 + v).  The largest eta of the full
colour + alpha + depth expectation is recorded with each scene (screened on the CPU oracle); a scene whose eta grows past 1.5 x that fails."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_alpha_abi import alpha_upstream, zero_colour_input
from tests.test_depth_abi import depth_colour_input, depth_upstream, z_row
from tests.test_gpu_batch_backward import _leaves, _settings, _t, make_scene

pytestmark = pytest.mark.gpu

W, H = 176, 112
# (P, V, D, M, cloud seed, scale_mult, recorded eta).  M = 0: colors_precomp (per-view colours).  Why these shapes: one Gaussian, one view /
# the ragged tail of the split kernel's group, V crosses BATCH_VIEWS = 8 / exactly one view chunk / the one-thread batch kernel, three chunks /
# M = 4 / per-view colours.
SCENES = [
    (1, 1, 0, 16, 3, 0.2, 2.4e-6),
    (129, 9, 1, 16, 4, 1.0, 1.4e-5),
    (2000, 8, 3, 16, 1406, 2.0, 5.2e-6),
    (257, 17, 0, 9, 811, 1.0, 4.2e-6),
    (2999, 9, 1, 4, 512, 2.0, 7.4e-6),
]
PRECOMP = (2999, 8, 0, 0, 616, 2.0, 5.3e-6)
ids = lambda cases: [f"P{c[0]}-V{c[1]}-D{c[2]}-M{c[3]}" for c in cases]
SUMMED = ("dL_dopacity", "dL_dmeans3D", "dL_dscales", "dL_drotations")          # summed over the views; every term takes part
COMBOS = {"colour": (False, False), "colour+alpha": (True, False), "colour+depth": (False, True), "colour+alpha+depth": (True, True)}
FULL = "colour+alpha+depth"


def upstream_maps(v):
    g_A = (np.random.Generator(np.random.PCG64(2024 + v)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    g_D = (np.random.Generator(np.random.PCG64(4048 + v)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    return g_A, g_D


@functools.lru_cache(maxsize=None)
def reference(P, V, D, M, seed, scale_mult):
    """The scene, its upstream gradients and, per oracle build, the three terms of the expectation for every view -- computed once per
    scene, read-only."""
    cloud, cams, dLs = make_scene(P, V, D, M, False, seed, scale_mult, False)
    colour_key = "dL_dsh" if M else "dL_dcolors"
    gAs, gDs = zip(*(upstream_maps(v) for v in range(V)))
    terms = {}
    alpha_maps, depth_maps, images, counts, visible = [], [], [], [], []
    for variant in ("f32", "f64"):
        per_view = []
        for v, cam in enumerate(cams):
            inp = util.scene_input(cloud, cam, "sh" if M else "precomp")
            c = util.oracle_run(inp, dLs[v], variant=variant)
            z = np.asarray(c["depths"])
            a = util.oracle_run(zero_colour_input(inp), alpha_upstream(gAs[v]), variant=variant)
            d = util.oracle_run(depth_colour_input(inp, z), depth_upstream(gDs[v]), variant=variant)
            for other in (a, d):                            # one compositing: the same pairs in all three frames
                assert np.array_equal(np.asarray(other["n_contrib"]), np.asarray(c["n_contrib"])), (variant, v)
            f = lambda r, k: np.asarray(r[k], np.float64).reshape(P, -1)
            t = {"colour": {k: f(c, k) for k in SUMMED + ("dL_dmeans2D", colour_key)},
                 "alpha": {k: f(a, k) for k in SUMMED + ("dL_dmeans2D",)},
                 "depth": {k: f(d, k) for k in SUMMED + ("dL_dmeans2D",)}}
            dz = f(d, "dL_dcolors")[:, 0]
            t["depth"]["dL_dmeans3D"] = t["depth"]["dL_dmeans3D"] + dz[:, None] * z_row(cam.viewmatrix)[None, :]
            per_view.append(t)
            if variant == "f32":
                alpha_maps.append(1.0 - np.asarray(c["final_T"], np.float64))
                depth_maps.append(np.asarray(d["color"], np.float64)[0])
                images.append(np.asarray(c["color"], np.float64))
                counts.append(int(c["num_rendered"]))
                visible.append(np.asarray(c["radii"]) > 0)
        terms[variant] = per_view
    dead = ~np.stack(visible).any(axis=0)
    return dict(cloud=cloud, cams=cams, dLs=dLs, gAs=gAs, gDs=gDs, terms=terms, alpha=alpha_maps, depth=depth_maps, images=images, counts=counts,
                colour_key=colour_key, dead=dead, P=P, V=V, D=D, M=M)


def expectation(ref, combo):
    """-> {"f32" / "f64": (summed parameter gradients {k: [P, n]}, per view {k: [P, n]})} for the upstream combination ``combo``"""
    with_alpha, with_depth = COMBOS[combo]
    out = {}
    for variant, per_view in ref["terms"].items():
        sums, views = {}, []
        for t in per_view:
            parts = [t["colour"]] + ([t["alpha"]] if with_alpha else []) + ([t["depth"]] if with_depth else [])
            for k in SUMMED:
                sums[k] = sums.get(k, 0.0) + sum(p[k] for p in parts)
            one = {"dL_dmeans2D": sum(p["dL_dmeans2D"] for p in parts)}
            if ref["M"]:
                sums["dL_dsh"] = sums.get("dL_dsh", 0.0) + t["colour"]["dL_dsh"]
            else:
                one["dL_dcolors"] = t["colour"]["dL_dcolors"]
            views.append(one)
        out[variant] = (sums, views)
    return out


def bar(e32, e64):
    eta = util.rel_l2(e32, e64)
    assert 2.0 * eta <= util.BAR_CAP, f"the scene's own fp32 noise ({eta:.3g}) is past the cap: replace the scene"
    return min(max(util.REL_TOL, 2.0 * eta), util.BAR_CAP), eta


def scene_eta(ref, combo=FULL):
    """the largest eta over the summed parameter gradients, every view's per-view gradients and both maps' reference (the maps: fp32 against
    fp64 of the frames they are read from is part of the colour frame's eta in the one-view suites; here the gradients decide)"""
    exp = expectation(ref, combo)
    (s32, v32), (s64, v64) = exp["f32"], exp["f64"]
    return max([util.rel_l2(s32[k], s64[k]) for k in s32] + [util.rel_l2(a[k], b[k]) for a, b in zip(v32, v64) for k in a])


def check(got_sums, got_views, ref, combo, what, scale=1.0):
    """got_sums {k: array}, got_views [{k: array}] against the fp32 expectation at the bar; ``scale``: the summed gradients hold that multiple of it
    (accumulated twice; the per-view tensors are written, never added to)"""
    exp = expectation(ref, combo)
    (s32, v32), (s64, v64) = exp["f32"], exp["f64"]
    worst = 0.0
    for k, e32 in s32.items():
        b, eta = bar(e32, s64[k])
        e = util.rel_l2(np.asarray(got_sums[k], np.float64).reshape(e32.shape) / scale, e32)
        print(f"{what} {k}: rel-L2 {e:.3e} (bar {b:.2e}, eta {eta:.2e})")
        assert e <= b, f"{what}: {k} rel-L2 {e:.3e} > {b:.2e}"
        worst = max(worst, e)
    for v, (one32, one64) in enumerate(zip(v32, v64)):
        for k, e32 in one32.items():
            b, eta = bar(e32, one64[k])
            a = np.asarray(got_views[v][k], np.float64).reshape(len(e32), -1)
            if k == "dL_dmeans2D":
                assert np.all(a[:, 2] == 0), (what, v)
                a = a[:, :e32.shape[1]] if e32.shape[1] < 3 else a
            e = util.rel_l2(a, e32)
            assert e <= b, f"{what}: view {v} {k} rel-L2 {e:.3e} > {b:.2e} (eta {eta:.2e})"
            worst = max(worst, e)
    return worst


def check_maps(alpha, depth, ref, what):
    tol = util.tolerance("color", None)
    for v in range(ref["V"]):
        if alpha is not None:
            e = util.rel_l2(alpha[v].detach().cpu().numpy().reshape(H, W), ref["alpha"][v])
            assert e <= tol, f"{what}: view {v} alpha rel-L2 {e:.3e}"
        if depth is not None:
            e = util.rel_l2(depth[v].detach().cpu().numpy().reshape(H, W), ref["depth"][v])
            assert e <= tol, f"{what}: view {v} depth rel-L2 {e:.3e}"


# ---- 1. the entry points on frames from _C.forward_views ----
class Frames:
    """The V views of a scene rendered by ONE _C.forward_views call into caller-allocated buffers; maps and backward passes on their state."""

    def __init__(self, ref, dev):
        from diff_gaussian_rasterization import _C
        self.ref, self.dev = ref, dev
        P, V, M, cloud = ref["P"], ref["V"], ref["M"], ref["cloud"]
        self.P, self.V, self.M, self.D = P, V, M, ref["D"]
        self.means, self.opac, self.scales, self.rots = (_t(cloud[k], dev) for k in ("means3D", "opacities", "scales", "rotations"))
        self.shs = _t(cloud["shs"], dev) if M else None
        self.colors = None if M else torch.stack([_t(util.scene_input(cloud, c, "precomp")["colors_precomp"], dev) for c in ref["cams"]])
        self.cap = max(ref["counts"]) + 256                 # (the HIP lists are the oracle's minus instances that cannot contribute)
        gb, bb, ib = _C.state_sizes(P, W, H, bool(M), True, self.cap)
        al = lambda n: (n + 255) // 256 * 256
        z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        self.buf = dict(images=z(V, 3, H, W), radii=z(V, P, dt=torch.int32), g2d=z(V, P, 3), gcol=z(V, P, 3), geom=z(V, al(gb), dt=torch.uint8),
                        binning=z(V, al(bb), dt=torch.uint8), img=z(V, al(ib), dt=torch.uint8), alpha=z(V, 1, H, W), depth=z(V, 1, H, W), dz=z(V, self.cap))
        self.cam = [{k: _t(getattr(c, k), dev) for k in ("viewmatrix", "projmatrix", "campos", "bg")} for c in ref["cams"]]
        self.dL = torch.stack([_t(d, dev) for d in ref["dLs"]])
        self.gA = torch.stack([_t(g, dev) for g in ref["gAs"]]).reshape(V, 1, H, W)
        self.gD = torch.stack([_t(g, dev) for g in ref["gDs"]]).reshape(V, 1, H, W)
        self.arr, self.xarr = _C.ViewArray(V), _C.ViewExtrasArray(V)
        for v, c in enumerate(ref["cams"]):
            a, b = self.arr[v], self.buf
            a.width, a.height, a.tan_fovx, a.tan_fovy = W, H, float(c.tanfovx), float(c.tanfovy)
            a.viewmatrix, a.projmatrix, a.campos, a.background = (self.cam[v][k].data_ptr() for k in ("viewmatrix", "projmatrix", "campos", "bg"))
            a.radii = a.radii_out = b["radii"][v].data_ptr()
            a.geom_buffer, a.binning_buffer, a.img_buffer = b["geom"][v].data_ptr(), b["binning"][v].data_ptr(), b["img"][v].data_ptr()
            a.geom_bytes, a.binning_bytes, a.img_bytes = gb, bb, ib
            a.out_color, a.dL_dmean2D, a.dL_dpix = b["images"][v].data_ptr(), b["g2d"][v].data_ptr(), self.dL[v].data_ptr()
            a.dL_dcolor = None if M else b["gcol"][v].data_ptr()
            a.colors_precomp = None if M else self.colors[v].data_ptr()
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.opt = _C.options(deterministic=True)
        _C.forward_views([self.stream], self.cap, P, self.D, M, self.means.data_ptr(), self.shs.data_ptr() if M else None, self.opac.data_ptr(),
                         self.scales.data_ptr(), 1.0, self.rots.data_ptr(), self.arr, V, opt=self.opt)

    def maps(self):
        from diff_gaussian_rasterization import _C
        for v in range(self.V):
            self.xarr[v].out_alpha, self.xarr[v].out_depth = self.buf["alpha"][v].data_ptr(), self.buf["depth"][v].data_ptr()
        self.buf["alpha"].fill_(float("nan")); self.buf["depth"].fill_(float("nan"))
        _C.outputs_views([self.stream], self.P, self.arr, self.xarr, self.V)
        return self.buf["alpha"], self.buf["depth"]

    def render_backward(self, combo):
        """the per-pixel half of every view with the combination's upstream gradients; dz scratch NaN-filled in front (the call zero-fills it)"""
        from diff_gaussian_rasterization import _C
        with_alpha, with_depth = COMBOS[combo]
        self.buf["dz"].fill_(float("nan"))
        for v in range(self.V):
            x = self.xarr[v]
            x.dL_dalpha = self.gA[v].data_ptr() if with_alpha else None
            x.dL_ddepth = self.gD[v].data_ptr() if with_depth else None
            x.dz_scratch = self.buf["dz"][v].data_ptr() if with_depth else None
        _C.backward_render_views_extras([self.stream], self.P, self.arr, self.xarr, self.V, opt=self.opt)

    def into(self, fill):
        P = self.P
        shapes = dict(means3D=(P, 3), opacities=(P, 1), scales=(P, 3), rotations=(P, 4), **({"sh": (P, self.M, 3)} if self.M else {}))
        return {k: fill(s) for k, s in shapes.items()}

    def gauss_backward(self, g, accumulate, ranges=None):
        """the per-Gaussian pass and, behind each range, the z-path pass of the depth gradient (a no-op without a depth gradient)"""
        from diff_gaussian_rasterization import _C
        for first, count in (ranges or [(0, self.P)]):
            _C.backward_batch_raw(self.stream, self.P, self.D, self.M, self.arr, self.V, self.means.data_ptr(), self.shs.data_ptr() if self.M else None,
                                  self.scales.data_ptr(), 1.0, self.rots.data_ptr(), g["opacities"].data_ptr(), g["means3D"].data_ptr(),
                                  g["sh"].data_ptr() if self.M else None, g["scales"].data_ptr(), g["rotations"].data_ptr(), accumulate, first=first, count=count)
            _C.backward_batch_depth_raw(self.stream, self.P, self.arr, self.xarr, self.V, g["means3D"].data_ptr(), first, count)
        torch.cuda.synchronize()

    def results(self, g):
        names = {"dL_dopacity": "opacities", "dL_dmeans3D": "means3D", "dL_dscales": "scales", "dL_drotations": "rotations", "dL_dsh": "sh"}
        sums = {k: g[n].cpu().numpy() for k, n in names.items() if n in g}
        views = [{"dL_dmeans2D": self.buf["g2d"][v].cpu().numpy(), **({} if self.M else {"dL_dcolors": self.buf["gcol"][v].cpu().numpy()})} for v in range(self.V)]
        return sums, views


@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,eta_rec", SCENES + [PRECOMP], ids=ids(SCENES + [PRECOMP]))
def test_entry_points_on_frames_of_forward_views(P, V, D, M, seed, scale_mult, eta_rec, gpu_device):
    ref = reference(P, V, D, M, seed, scale_mult)
    eta = scene_eta(ref)
    assert eta <= 1.5 * eta_rec, f"the scene's own fp32 noise grew: eta {eta:.3g} > 1.5 x {eta_rec:.3g}"
    fr = Frames(ref, gpu_device)
    torch.cuda.synchronize()
    radii = fr.buf["radii"].cpu().numpy()
    dead = ~(radii > 0).any(axis=0)
    assert np.array_equal(dead, ref["dead"])
    if P >= 97:
        assert dead[::97].all() and dead.sum() < P // 2
    alpha, depth = fr.maps()
    torch.cuda.synchronize()
    check_maps(alpha, depth, ref, "tgs_outputs_views")
    assert np.array_equal(fr.maps()[0].cpu().numpy(), alpha.cpu().numpy())
    rep = {"eta": eta}
    gen = torch.Generator(device=gpu_device).manual_seed(seed)
    for combo, (with_alpha, with_depth) in COMBOS.items():
        fr.render_backward(combo)
        got = fr.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
        fr.gauss_backward(got, accumulate=False)
        sums, views = fr.results(got)
        for k, a in sums.items():
            assert np.isfinite(a).all(), f"{combo} {k}: store mode left elements unwritten"
            assert np.all(a[dead] == 0), f"{combo} {k}: Gaussians culled in every view must be exactly 0"
        for v, d in enumerate(views):
            for k, a in d.items():
                assert np.isfinite(a).all() and np.all(a[~(radii[v] > 0)] == 0), (combo, v, k)
        rep[combo] = check(sums, views, ref, combo, f"store [{combo}]")
        if with_depth:
            assert torch.isfinite(fr.buf["dz"]).all(), "dz scratch was not zero-filled"
        # accumulate = store + what the buffers held
        base = fr.into(lambda s: torch.randn(s, device=gpu_device, generator=gen) * 1e-3)
        acc = {k: b.clone() for k, b in base.items()}
        fr.gauss_backward(acc, accumulate=True)
        for k in acc:
            assert util.rel_l2(acc[k].cpu().numpy(), (base[k].double() + got[k].double()).cpu().numpy()) <= 1e-6, (combo, k)
        if with_depth:
            # two runs give the same bits (deterministic per-pixel kernel, no float atomics and a fixed order in the depth passes) ...
            fr.render_backward(combo)
            again = fr.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
            fr.gauss_backward(again, accumulate=False)
            for k in got:
                assert torch.equal(got[k], again[k]), (combo, k, "two runs differ")
            # ... and ranges on multiples of 256 give the bits of the whole-range call
            if P > 256:
                cut = [0, 256] + ([P // 512 * 256] if P // 512 * 256 > 256 else []) + [P]
                parts = fr.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
                fr.gauss_backward(parts, accumulate=False, ranges=[(a, b - a) for a, b in zip(cut[:-1], cut[1:])])
                for k in got:
                    assert torch.equal(got[k], parts[k]), (combo, k, "ranges differ from the whole launch")
    util.record_parity(f"batch_extras/entry-P{P}-V{V}-D{D}-M{M}", rep)


# ---- 2. run_views on every route ----
def _batch_setup(ref, dev, level_major=False):
    from youreditableavatar_amd.multiview import FlatGradients
    names = ("means3D", "opacities", "scales", "rotations") + (("shs",) if ref["M"] else ())
    L = _leaves(ref["cloud"], dev, names)
    flat = FlatGradients([L[n] for n in names])
    settings = [_settings(c, ref["D"], dev) for c in ref["cams"]]
    colors = None if ref["M"] else torch.stack([_t(util.scene_input(ref["cloud"], c, "precomp")["colors_precomp"], dev) for c in ref["cams"]])
    up = dict(dL=torch.stack([_t(d, dev) for d in ref["dLs"]]), gA=torch.stack([_t(g, dev) for g in ref["gAs"]]).reshape(-1, 1, H, W),
              gD=torch.stack([_t(g, dev) for g in ref["gDs"]]).reshape(-1, 1, H, W))
    return L, flat, settings, colors, up


def _run(batch, ref, L, settings, colors, kind, upstream, **kw):
    """one run_views call; ``upstream(v or None, image(s), *maps) -> what the callable returns`` serves both kinds of callable"""
    args = (settings, L["means3D"], L["opacities"], L.get("shs"), L["scales"], L["rotations"])
    if kind == "batch":
        return batch.run_views(*args, lambda images, *maps: upstream(None, images, *maps), colors_precomp=colors, **kw)
    return batch.run_views(*args, None, colors_precomp=colors, upstream_view=lambda v, image, *maps: upstream(v, image, *maps), **kw)


def _grads(L, batch, ref):
    names = {"dL_dopacity": "opacities", "dL_dmeans3D": "means3D", "dL_dscales": "scales", "dL_drotations": "rotations", "dL_dsh": "shs"}
    sums = {k: L[n].grad.detach().cpu().numpy() for k, n in names.items() if n in L}
    views = [{"dL_dmeans2D": batch.viewspace_grads[v].cpu().numpy(), **({} if ref["M"] else {"dL_dcolors": batch.color_grads[v].cpu().numpy()})}
             for v in range(ref["V"])]
    return sums, views


def full_upstream(up):
    def f(v, images, alpha, depth):
        assert tuple(alpha.shape[-3:]) == (1, H, W) and tuple(depth.shape[-3:]) == (1, H, W) and alpha.dim() == depth.dim() == (3 if v is not None else 4)
        return (up["dL"], up["gA"], up["gD"]) if v is None else (up["dL"][v], up["gA"][v], up["gD"][v])
    return f


RUN_SCENES = [SCENES[1], SCENES[2], PRECOMP]


@pytest.mark.parametrize("config", ["default", "split4"])
@pytest.mark.parametrize("kind", ["batch", "view"])
@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,eta_rec", RUN_SCENES, ids=ids(RUN_SCENES))
def test_run_views_with_alpha_and_depth(P, V, D, M, seed, scale_mult, eta_rec, kind, config, gpu_device):
    """The first call of a SyncFreeBatch (synchronous route) and the second and third (pooled route): maps and gradients at the bar;
    accumulate=False with grad_chunks=3 and a recording on_chunk, then accumulate=True on top of it (twice the gradient)."""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    ref = reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, up = _batch_setup(ref, gpu_device)
    batch = SyncFreeBatch(granule=256, deterministic=True, **(dict(split=True, streams=4) if config == "split4" else {}))
    kw = dict(return_alpha=True, return_depth=True)
    rep = {}
    # call 1: no bound yet -- synchronous frames, the extended one-view backward
    flat.flat.fill_(float("nan"))
    images, alpha, depth = _run(batch, ref, L, settings, colors, kind, full_upstream(up), accumulate=False, **kw)
    torch.cuda.synchronize()
    assert tuple(alpha.shape) == tuple(depth.shape) == (V, 1, H, W) and tuple(images.shape) == (V, 3, H, W)
    check_maps(alpha, depth, ref, "first call")
    rep["first"] = check(*_grads(L, batch, ref), ref, FULL, f"run_views first call [{kind}, {config}]")
    assert batch.capacity() is not None
    # call 2: the pooled route, stored, three ranges
    calls = []
    flat.flat.fill_(float("nan"))
    images, alpha, depth = _run(batch, ref, L, settings, colors, kind, full_upstream(up), accumulate=False, grad_chunks=3,
                                on_chunk=lambda first, count: calls.append((first, count)), **kw)
    torch.cuda.synchronize()
    assert batch.rejected == 0 and batch._pool is not None and alpha.data_ptr() == batch._pool["alpha"].data_ptr()
    chunks = max(1, min(3, (P + 255) // 256))
    per = ((P + chunks - 1) // chunks + 255) // 256 * 256
    assert calls == [(first, min(per, P - first)) for first in range(0, P, per)]
    check_maps(alpha, depth, ref, "second call")
    for v in range(V):
        assert util.rel_l2(images[v].cpu().numpy(), ref["images"][v]) <= util.REL_TOL
    rep["pooled"] = check(*_grads(L, batch, ref), ref, FULL, f"run_views pooled [{kind}, {config}]")
    stored = flat.flat.clone()
    # call 3: the pooled route again, added to what call 2 stored
    _run(batch, ref, L, settings, colors, kind, full_upstream(up), accumulate=True, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == 0
    assert util.rel_l2(flat.flat.cpu().numpy(), 2.0 * stored.double().cpu().numpy()) <= 1e-6
    rep["accumulated"] = check(*_grads(L, batch, ref), ref, FULL, f"run_views pooled, accumulate [{kind}, {config}]", scale=2.0)
    util.record_parity(f"batch_extras/run_views-P{P}-V{V}-M{M}-{kind}-{config}", rep)


# ---- 3. forced re-rendering ----
@pytest.mark.parametrize("kind", ["batch", "view"])
def test_rejected_frames_are_rendered_again_with_their_maps(kind, gpu_device):
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, _eta = SCENES[2]
    ref = reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, up = _batch_setup(ref, gpu_device)
    batch = SyncFreeBatch(granule=64, deterministic=True)
    kw = dict(return_alpha=True, return_depth=True)
    flat.zero_()
    _run(batch, ref, L, settings, colors, kind, full_upstream(up), **kw)                  # the learning batch
    assert batch.capacity() is not None and batch.rejected == 0
    assert min(ref["counts"]) > 4 * 64
    batch.bound = 1                                         # capacity 64: below every view's instance count
    seen = []

    def upstream(v, images, alpha, depth):
        seen.append((alpha.detach().clone(), depth.detach().clone()))
        return full_upstream(up)(v, images, alpha, depth)

    flat.flat.fill_(float("nan"))
    images, alpha, depth = _run(batch, ref, L, settings, colors, kind, upstream, accumulate=False, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == V
    # the rejected frames rendered the background and zero maps; the second round of upstream calls saw the corrected ones
    first = seen[0]
    assert bool((first[0] == 0).all()) and bool((first[1] == 0).all())
    assert len(seen) == (2 if kind == "batch" else 2 * V)
    check_maps(alpha, depth, ref, "re-rendered")              # in the returned (pooled) buffers
    assert alpha.data_ptr() == batch._pool["alpha"].data_ptr() and depth.data_ptr() == batch._pool["depth"].data_ptr()
    for v in range(V):
        assert util.rel_l2(images[v].cpu().numpy(), ref["images"][v]) <= util.REL_TOL
    check(*_grads(L, batch, ref), ref, FULL, f"run_views re-rendered [{kind}]")
    # the bound has been learned again: the next call is sync-free and complete
    flat.flat.fill_(float("nan"))
    _run(batch, ref, L, settings, colors, kind, full_upstream(up), accumulate=False, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == V
    check(*_grads(L, batch, ref), ref, FULL, f"run_views after re-rendering [{kind}]")


# ---- 4. flags off and gradients absent ----
def _pooled_grads(ref, dev, kind, upstream, **kw):
    """the parameter gradients (flat buffer), dL_dmeans2D and the returned maps of the third call (pooled route) of a fresh deterministic SyncFreeBatch"""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    L, flat, settings, colors, up = _batch_setup(ref, dev)
    batch = SyncFreeBatch(granule=256, deterministic=True)
    for _ in range(3):
        flat.flat.fill_(float("nan"))
        out = _run(batch, ref, L, settings, colors, kind, upstream(up), accumulate=False, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == 0
    return flat.flat.clone(), batch.viewspace_grads.clone(), out, batch


@pytest.mark.parametrize("kind", ["batch", "view"])
def test_flags_off_and_absent_gradients_change_nothing(kind, gpu_device):
    P, V, D, M, seed, scale_mult, _eta = SCENES[2]
    ref = reference(P, V, D, M, seed, scale_mult)
    pick = lambda t, v: t if v is None else t[v]
    plain = lambda up: (lambda v, images: pick(up["dL"], v))
    g0, m0, out0, batch0 = _pooled_grads(ref, gpu_device, kind, plain)
    assert torch.is_tensor(out0) and "alpha" not in batch0._pool and "xarr" not in batch0._pool and len(batch0._pool["key"]) == 8
    both = dict(return_alpha=True, return_depth=True)
    # both maps returned, neither used: the bits of the call without the flags
    g, m, out, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, a, d: (pick(up["dL"], v), None, None)), **both)
    assert isinstance(out, tuple) and len(out) == 3 and torch.equal(g, g0) and torch.equal(m, m0) and torch.equal(out[0], out0)
    # a zero depth gradient runs the depth kernels and adds zeros
    g, m, _o, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, a, d: (pick(up["dL"], v), None, torch.zeros_like(pick(up["gD"], v)))), **both)
    assert torch.equal(g, g0) and torch.equal(m, m0)
    # one gradient alone with both flags == the run that asked for that map alone
    gA1, mA1, outA, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, a: (pick(up["dL"], v), pick(up["gA"], v))), return_alpha=True)
    gA2, mA2, _o, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, a, d: (pick(up["dL"], v), pick(up["gA"], v), None)), **both)
    assert len(outA) == 2 and torch.equal(gA1, gA2) and torch.equal(mA1, mA2) and not torch.equal(gA1, g0)
    gD1, mD1, outD, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, d: (pick(up["dL"], v), pick(up["gD"], v))), return_depth=True)
    gD2, mD2, _o, _b = _pooled_grads(ref, gpu_device, kind, lambda up: (lambda v, images, a, d: (pick(up["dL"], v), None, pick(up["gD"], v))), **both)
    assert len(outD) == 2 and torch.equal(gD1, gD2) and torch.equal(mD1, mD2) and not torch.equal(gD1, g0)
    check_maps(outA[1], None, ref, "alpha alone")
    check_maps(None, outD[1], ref, "depth alone")
    # a [1,H,W] gradient from the batch callable is shared by all views
    if kind == "batch":
        shared = lambda up: (lambda v, images, a, d: (up["dL"], up["gA"][0], up["gD"][0]))
        expanded = lambda up: (lambda v, images, a, d: (up["dL"], up["gA"][:1].expand(V, 1, H, W), up["gD"][:1].expand(V, 1, H, W)))
        gs, ms, _o, _b = _pooled_grads(ref, gpu_device, kind, shared, **both)
        ge, me, _o, _b = _pooled_grads(ref, gpu_device, kind, expanded, **both)
        assert torch.equal(gs, ge) and torch.equal(ms, me)


# ---- 5. wrong upstream returns ----
@pytest.mark.parametrize("kind", ["batch", "view"])
def test_wrong_upstream_returns_raise_and_leave_the_batch_usable(kind, gpu_device):
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, _eta = SCENES[1]
    ref = reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, up = _batch_setup(ref, gpu_device)
    pick = lambda t, v: t if v is None else t[v]
    wrong = {
        "a bare tensor": lambda v, images, a, d: pick(up["dL"], v),
        "arity": lambda v, images, a, d: (pick(up["dL"], v), pick(up["gA"], v)),
        "[3,H,W]": lambda v, images, a, d: (pick(up["dL"], v), up["dL"][0], None),
        "float64": lambda v, images, a, d: (pick(up["dL"], v), None, pick(up["gD"], v).double()),
    }
    batch = SyncFreeBatch(granule=256, deterministic=True)
    kw = dict(return_alpha=True, return_depth=True, accumulate=False)
    for route in ("synchronous", "pooled"):
        for what, f in wrong.items():
            with pytest.raises(RuntimeError, match="upstream"):
                _run(batch, ref, L, settings, colors, kind, f, **kw)
        flat.flat.fill_(float("nan"))
        _images, alpha, depth = _run(batch, ref, L, settings, colors, kind, full_upstream(up), **kw)
        torch.cuda.synchronize()
        assert (batch.capacity() is not None) and batch.rejected == 0
        check_maps(alpha, depth, ref, f"after the wrong returns ({route})")
        check(*_grads(L, batch, ref), ref, FULL, f"after the wrong returns ({route}) [{kind}]")
    assert batch._pool is not None


# ---- 6. the example ----
def test_example_fits_masks_and_depth_maps_of_several_views(gpu_device):
    """examples/fit_views_silhouette_depth.py at a small size: the loss falls (what test_example_fits_a_depth_map asks of fit_depth.py)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fit_views_silhouette_depth", os.path.join(util.ROOT, "examples", "fit_views_silhouette_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    vals = mod.run(steps=40, P=400, W=64, H=48, views=4, log=lines.append)
    print("\n".join(lines))
    assert len(vals) == 41 and all(np.isfinite(vals)) and vals[-1] < vals[0]
