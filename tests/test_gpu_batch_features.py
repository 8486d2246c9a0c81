"""Feature channels in the whole-batch path: tgs_features_views, tgs_backward_render_views_features_opt, tgs_backward_batch_features_range
(k_feat_bwd_gauss_views) through the _C bindings, and SyncFreeBatch.run_views(features=) on every route.

Yardstick: the CPU oracle alone, composed as tests/test_gpu_batch_extras.py (colour, alpha, depth: its ``reference``) and
tests/test_gpu_features.py (features: ``oracle_features`` of tests/test_features_abi.py) compose it.  Per view the feature map is the oracle's
feature-colour frames, the through-alpha term their summed gradients, dL_dfeatures their dL_dcolors; oracle_features asserts that those
frames blend the n_contrib of the colour frame.  Over the views dL_dfeatures and the parameter gradients are summed in float64; dL_dmeans2D
(and dL_dcolors with per-view colours) are compared per view.  Maps at util.tolerance("color", None).

Bar: the frozen one, per tensor min(max(1e-4, 2 eta), 1e-3) with eta = rel_l2(that expectation from the fp32 oracle, from the fp64 oracle),
computed here; the 1e-3 cap is a condition (asserted), no failure budget.  Scenes: tests.test_gpu_batch_backward.make_scene, 176 x 112 (the
clouds and cameras of tests/test_gpu_batch_extras.py, so its cached reference serves both files); per-view g_F = standard_normal((C,H,W)) /
(H W) from PCG64(6072 + v), features standard_normal from PCG64(515 + C).  The largest eta of the colour + features and the colour + alpha +
depth + features expectations is recorded with each scene (screened on the CPU oracle: 2 eta is 50 times below the cap in all of them); a
scene whose eta grows past 1.5 x that fails."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_features_abi import make_features, oracle_features
from tests.test_gpu_batch_backward import _leaves, _settings, _t
from tests.test_gpu_batch_extras import COMBOS, FULL, PRECOMP, SCENES, SUMMED, Frames, bar, check_maps, expectation, reference

pytestmark = pytest.mark.gpu

W, H = 176, 112
# the scenes of tests/test_gpu_batch_extras.py with a channel count each: (P, V, D, M, cloud seed, scale_mult, C, recorded eta).  What they cross:
#   P1    one Gaussian, one view, one channel (the narrow per-pixel kernel, scalar loads in the per-Gaussian pass)
#   P129  V crosses BATCH_VIEWS = 8: a second launch that adds, a partly filled group; C % 4 != 0
#   P2000 exactly one view chunk; two channel groups; 16-byte loads
#   P257  three view chunks; a group plus one channel; P one past PRE_BLOCK (two ranges)
#   P2999 one full narrow group / (per-view colours) one full wide group
CHANNELS = (1, 5, 16, 9, 4)
FSCENES = [s[:6] + (C, eta) for s, C, eta in zip(SCENES, CHANNELS, (6.9e-6, 8.3e-6, 5.2e-6, 3.9e-6, 5.6e-6))]
FPRECOMP = PRECOMP[:6] + (8, 4.5e-6)
ids = lambda cases: [f"P{c[0]}-V{c[1]}-D{c[2]}-M{c[3]}-C{c[6]}" for c in cases]
FCOMBOS = {"colour+features": "colour", "colour+alpha+depth+features": FULL}         # -> the combination of the extras' expectation beside it
FFULL = "colour+alpha+depth+features"


def upstream_features(v, C):
    return (np.random.Generator(np.random.PCG64(6072 + v)).standard_normal((C, H, W)) / (H * W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def feature_reference(P, V, D, M, seed, scale_mult, C):
    """The features, their upstream gradients and, per oracle build and view, the feature terms of the expectation -- computed once per
    scene, read-only; ["base"]: the colour / alpha / depth reference of the same scene."""
    base = reference(P, V, D, M, seed, scale_mult)
    F = make_features(P, C, seed=515 + C)
    gFs = [upstream_features(v, C) for v in range(V)]
    terms, fmaps = {}, []
    for variant in ("f32", "f64"):
        per_view = []
        for v, cam in enumerate(base["cams"]):
            inp = util.scene_input(base["cloud"], cam, "sh" if M else "precomp")
            n_contrib = np.asarray(util.oracle_run(inp, None, variant=variant)["n_contrib"])
            fmap, dF, summed = oracle_features(inp, F, gFs[v], variant, n_contrib=n_contrib)
            t = {k: np.asarray(summed[k], np.float64).reshape(P, -1) for k in SUMMED + ("dL_dmeans2D",)}
            t["dL_dfeatures"] = dF
            per_view.append(t)
            if variant == "f32":
                fmaps.append(np.asarray(fmap, np.float64))
        terms[variant] = per_view
    return dict(base=base, F=F, gFs=gFs, terms=terms, fmaps=fmaps, C=C, P=P, V=V, D=D, M=M)


def expectation_f(fref, combo, fviews=None, with_dF=True):
    """-> {"f32" / "f64": (summed gradients {k: [P, n]}, per view {k: [P, n]})}: the extras' expectation of ``FCOMBOS[combo]`` plus the feature
    terms of the views ``fviews`` (None: all); dL_dfeatures joins the summed ones (``with_dF``)"""
    fviews = range(fref["V"]) if fviews is None else fviews
    exp = expectation(fref["base"], FCOMBOS[combo])
    out = {}
    for variant, (sums, views) in exp.items():
        sums, views = dict(sums), [dict(one) for one in views]
        dF = np.zeros((fref["P"], fref["C"]), np.float64)
        for v in fviews:
            t = fref["terms"][variant][v]
            for k in SUMMED:
                sums[k] = sums[k] + t[k]
            views[v]["dL_dmeans2D"] = views[v]["dL_dmeans2D"] + t["dL_dmeans2D"]
            dF = dF + t["dL_dfeatures"]
        if with_dF:
            sums["dL_dfeatures"] = dF
        out[variant] = (sums, views)
    return out


def scene_eta(fref):
    """the largest eta over both upstream combinations: the summed gradients (dL_dfeatures among them) and every view's per-view gradients"""
    worst = 0.0
    for combo in FCOMBOS:
        (s32, v32), (s64, v64) = (lambda e: (e["f32"], e["f64"]))(expectation_f(fref, combo))
        worst = max([worst] + [util.rel_l2(s32[k], s64[k]) for k in s32] + [util.rel_l2(a[k], b[k]) for a, b in zip(v32, v64) for k in a])
    return worst


def check(got_sums, got_views, exp, what, scale=1.0):
    """got_sums {k: array}, got_views [{k: array}] against the fp32 expectation ``exp`` at the bar; ``scale``: the summed gradients hold that
    multiple of it (accumulated; the per-view tensors are written, never added to)"""
    (s32, v32), (s64, v64) = exp["f32"], exp["f64"]
    assert set(s32) <= set(got_sums), sorted(set(s32) - set(got_sums))
    for k, e32 in s32.items():
        b, eta = bar(e32, s64[k])
        e = util.rel_l2(np.asarray(got_sums[k], np.float64).reshape(e32.shape) / scale, e32)
        print(f"{what} {k}: rel-L2 {e:.3e} (bar {b:.2e}, eta {eta:.2e})")
        assert e <= b, f"{what}: {k} rel-L2 {e:.3e} > {b:.2e}"
    for v, (one32, one64) in enumerate(zip(v32, v64)):
        for k, e32 in one32.items():
            b, eta = bar(e32, one64[k])
            a = np.asarray(got_views[v][k], np.float64).reshape(len(e32), -1)
            if k == "dL_dmeans2D":
                assert np.all(a[:, 2] == 0), (what, v)
                a = a[:, :e32.shape[1]] if e32.shape[1] < 3 else a
            e = util.rel_l2(a, e32)
            assert e <= b, f"{what}: view {v} {k} rel-L2 {e:.3e} > {b:.2e} (eta {eta:.2e})"


def check_fmaps(fmap, fref, what, views=None):
    tol = util.tolerance("color", None)
    for v in (range(fref["V"]) if views is None else views):
        e = util.rel_l2(fmap[v].detach().cpu().numpy().reshape(fref["C"], H, W), fref["fmaps"][v])
        assert e <= tol, f"{what}: view {v} feature map rel-L2 {e:.3e}"


# ---- 1. the entry points on frames from _C.forward_views ----
class FFrames(Frames):
    """Frames with the third per-view array; ``n_streams`` > 1: the views are rendered again over that many streams (view k on stream
    k mod n), and maps and per-pixel backwards follow each view on its stream."""

    def __init__(self, fref, dev, n_streams):
        from diff_gaussian_rasterization import _C
        from youreditableavatar_amd import multiview as mv
        super().__init__(fref["base"], dev)
        self.fref, self.C = fref, fref["C"]
        V, C = self.V, self.C
        self.F = _t(fref["F"], dev)
        self.gF = torch.stack([_t(g, dev) for g in fref["gFs"]])
        self.buf.update(fmap=torch.zeros((V, C, H, W), device=dev), fscratch=torch.zeros((V, self.cap * C), device=dev))
        self.farr = _C.ViewFeaturesArray(V)
        for v in range(V):
            self.farr[v].C, self.farr[v].features = C, self.F.data_ptr()
        self.main = torch.cuda.current_stream(dev)
        self.lanes = mv._lanes(self.main, min(n_streams, V))
        self.handles = [st.cuda_stream for st in self.lanes]
        self._fork, self._join = mv._fork, mv._join
        if len(self.lanes) > 1:
            self._fork(self.lanes)
            _C.forward_views(self.handles, self.cap, self.P, self.D, self.M, self.means.data_ptr(), self.shs.data_ptr() if self.M else None, self.opac.data_ptr(),
                             self.scales.data_ptr(), 1.0, self.rots.data_ptr(), self.arr, V, opt=self.opt)
            self._join(self.lanes)

    def fmaps(self):
        from diff_gaussian_rasterization import _C
        self.buf["fmap"].fill_(float("nan"))
        for v in range(self.V):
            self.farr[v].out_features = self.buf["fmap"][v].data_ptr()
        self._fork(self.lanes)
        _C.features_views(self.handles, self.P, self.arr, self.farr, self.V)
        self._join(self.lanes)
        return self.buf["fmap"]

    def render_backward_f(self, combo, fviews=None):
        """the per-pixel half of every view: colour (+ alpha + depth), then the features' share for the views ``fviews`` (None: all); both
        scratches NaN-filled in front (the call zero-fills them)"""
        from diff_gaussian_rasterization import _C
        with_alpha, with_depth = COMBOS[FCOMBOS[combo]]
        self.buf["dz"].fill_(float("nan")); self.buf["fscratch"].fill_(float("nan"))
        for v in range(self.V):
            x, f = self.xarr[v], self.farr[v]
            x.dL_dalpha = self.gA[v].data_ptr() if with_alpha else None
            x.dL_ddepth = self.gD[v].data_ptr() if with_depth else None
            x.dz_scratch = self.buf["dz"][v].data_ptr() if with_depth else None
            on = fviews is None or v in fviews
            f.dL_dfeature_map = self.gF[v].data_ptr() if on else None
            f.feature_scratch = self.buf["fscratch"][v].data_ptr() if on else None
        self._fork(self.lanes)
        _C.backward_render_views_features(self.handles, self.P, self.arr, self.xarr if (with_alpha or with_depth) else None, self.farr, self.V, opt=self.opt)
        self._join(self.lanes)

    def into_f(self, fill):
        return dict(self.into(fill), features=fill((self.P, self.C)))

    def gauss_backward_f(self, g, accumulate, ranges=None):
        from diff_gaussian_rasterization import _C
        for first, count in (ranges or [(0, self.P)]):
            _C.backward_batch_raw(self.stream, self.P, self.D, self.M, self.arr, self.V, self.means.data_ptr(), self.shs.data_ptr() if self.M else None,
                                  self.scales.data_ptr(), 1.0, self.rots.data_ptr(), g["opacities"].data_ptr(), g["means3D"].data_ptr(),
                                  g["sh"].data_ptr() if self.M else None, g["scales"].data_ptr(), g["rotations"].data_ptr(), accumulate, first=first, count=count)
            _C.backward_batch_depth_raw(self.stream, self.P, self.arr, self.xarr, self.V, g["means3D"].data_ptr(), first, count)
            _C.backward_batch_features_raw(self.stream, self.P, self.arr, self.farr, self.V, g["features"].data_ptr(), accumulate, first, count)
        torch.cuda.synchronize()

    def results_f(self, g):
        sums, views = self.results(g)
        sums["dL_dfeatures"] = g["features"].cpu().numpy()
        return sums, views


@pytest.mark.parametrize("n_streams", [1, 4])
@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,C,eta_rec", FSCENES + [FPRECOMP], ids=ids(FSCENES + [FPRECOMP]))
def test_entry_points_on_frames_of_forward_views(P, V, D, M, seed, scale_mult, C, eta_rec, n_streams, gpu_device):
    fref = feature_reference(P, V, D, M, seed, scale_mult, C)
    eta = scene_eta(fref)
    print(f"scene eta {eta:.3e} (recorded {eta_rec:.3e})")
    assert eta <= 1.5 * eta_rec, f"the scene's own fp32 noise grew: eta {eta:.3g} > 1.5 x {eta_rec:.3g}"
    fr = FFrames(fref, gpu_device, n_streams)
    torch.cuda.synchronize()
    nan = lambda s: torch.full(s, float("nan"), device=gpu_device)
    radii = fr.buf["radii"].cpu().numpy()
    dead = ~(radii > 0).any(axis=0)
    assert np.array_equal(dead, fref["base"]["dead"])
    fmap = fr.fmaps()
    torch.cuda.synchronize()
    assert torch.isfinite(fmap).all()
    check_fmaps(fmap, fref, "tgs_features_views")
    for combo in FCOMBOS:
        exp = expectation_f(fref, combo)
        fr.render_backward_f(combo)
        got = fr.into_f(nan)
        fr.gauss_backward_f(got, accumulate=False)
        assert torch.isfinite(fr.buf["fscratch"]).all(), "the feature scratch was not zero-filled"
        sums, views = fr.results_f(got)
        for k, a in sums.items():
            assert np.isfinite(a).all(), f"{combo} {k}: store mode left elements unwritten"
            assert np.all(a[dead] == 0), f"{combo} {k}: Gaussians visible in no view must be exactly 0"
        check(sums, views, exp, f"store [{combo}, {n_streams} streams]")
        stored = {k: t.clone() for k, t in got.items()}
        # two runs give the same bits (deterministic per-pixel kernel, no float atomics and a fixed order) ...
        fr.render_backward_f(combo)
        again = fr.into_f(nan)
        fr.gauss_backward_f(again, accumulate=False)
        for k in stored:
            assert torch.equal(stored[k], again[k]), (combo, k, "two runs differ")
        # ... and the range [0, 256) plus the rest gives the bits of the whole-range call
        if P > 256:
            parts = fr.into_f(nan)
            fr.gauss_backward_f(parts, accumulate=False, ranges=[(0, 256), (256, P - 256)])
            for k in stored:
                assert torch.equal(stored[k], parts[k]), (combo, k, "ranges differ from the whole launch")
        # accumulate: twice on top of the store is three times the expectation
        fr.gauss_backward_f(got, accumulate=True)
        fr.gauss_backward_f(got, accumulate=True)
        sums3, _views = fr.results_f(got)
        assert np.all(sums3["dL_dfeatures"][dead] == 0)
        check(sums3, views, exp, f"store + 2 x accumulate [{combo}, {n_streams} streams]", scale=3.0)
    # a feature gradient in the even views only: the odd ones add nothing, anywhere
    if V > 1:
        even = list(range(0, V, 2))
        fr.render_backward_f("colour+features", fviews=even)
        got = fr.into_f(nan)
        fr.gauss_backward_f(got, accumulate=False)
        check(*fr.results_f(got), expectation_f(fref, "colour+features", fviews=even), f"even views [{n_streams} streams]")
    # no view with a gradient: store zero-fills the range, accumulate leaves it alone; the rest is the colour's backward
    fr.render_backward_f("colour+features", fviews=[])
    got = fr.into_f(nan)
    fr.gauss_backward_f(got, accumulate=False)
    assert bool((got["features"] == 0).all())
    keep = torch.randn((P, C), device=gpu_device)
    got["features"].copy_(keep)
    fr.gauss_backward_f({**fr.into_f(nan), "features": got["features"]}, accumulate=True)
    assert torch.equal(got["features"], keep)


# ---- 2. run_views on every route ----
def _batch_setup(fref, dev, requires_grad=True):
    from youreditableavatar_amd.multiview import FlatGradients
    ref = fref["base"]
    names = ("means3D", "opacities", "scales", "rotations") + (("shs",) if ref["M"] else ())
    L = _leaves(ref["cloud"], dev, names)
    flat = FlatGradients([L[n] for n in names])
    settings = [_settings(c, ref["D"], dev) for c in ref["cams"]]
    colors = None if ref["M"] else torch.stack([_t(util.scene_input(ref["cloud"], c, "precomp")["colors_precomp"], dev) for c in ref["cams"]])
    up = dict(dL=torch.stack([_t(d, dev) for d in ref["dLs"]]), gA=torch.stack([_t(g, dev) for g in ref["gAs"]]).reshape(-1, 1, H, W),
              gD=torch.stack([_t(g, dev) for g in ref["gDs"]]).reshape(-1, 1, H, W), gF=torch.stack([_t(g, dev) for g in fref["gFs"]]))
    F = _t(fref["F"], dev).requires_grad_(requires_grad)
    if requires_grad:
        F.grad = torch.full_like(F, float("nan"))
    return L, flat, settings, colors, up, F


def _run(batch, L, settings, colors, kind, upstream, **kw):
    args = (settings, L["means3D"], L["opacities"], L.get("shs"), L["scales"], L["rotations"])
    if kind == "batch":
        return batch.run_views(*args, lambda images, *maps: upstream(None, images, *maps), colors_precomp=colors, **kw)
    return batch.run_views(*args, None, colors_precomp=colors, upstream_view=lambda v, image, *maps: upstream(v, image, *maps), **kw)


def _grads(L, batch, fref, F=None):
    ref = fref["base"]
    names = {"dL_dopacity": "opacities", "dL_dmeans3D": "means3D", "dL_dscales": "scales", "dL_drotations": "rotations", "dL_dsh": "shs"}
    sums = {k: L[n].grad.detach().cpu().numpy() for k, n in names.items() if n in L}
    if F is not None and F.grad is not None:
        sums["dL_dfeatures"] = F.grad.detach().cpu().numpy()
    views = [{"dL_dmeans2D": batch.viewspace_grads[v].cpu().numpy(), **({} if ref["M"] else {"dL_dcolors": batch.color_grads[v].cpu().numpy()})}
             for v in range(ref["V"])]
    return sums, views


def upstream_of(up, C, extras, fviews=None):
    """the callable's body for both kinds: checks what it is handed, returns the recorded gradients (the feature gradient of a view outside
    ``fviews`` is None)"""
    def f(v, images, *maps):
        assert len(maps) == (3 if extras else 1)
        d = 3 if v is not None else 4
        for m in maps[:-1]:
            assert tuple(m.shape[-3:]) == (1, H, W) and m.dim() == d
        assert tuple(maps[-1].shape[-3:]) == (C, H, W) and maps[-1].dim() == d
        pick = lambda t: t if v is None else t[v]
        gF = pick(up["gF"]) if (fviews is None or v is None or v in fviews) else None
        return (pick(up["dL"]),) + ((pick(up["gA"]), pick(up["gD"])) if extras else ()) + (gF,)
    return f


RUN_SCENES = [FSCENES[1], FSCENES[2], FPRECOMP]


@pytest.mark.parametrize("extras", [False, True], ids=["features", "alpha+depth+features"])
@pytest.mark.parametrize("kind", ["batch", "view"])
@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,C,eta_rec", RUN_SCENES, ids=ids(RUN_SCENES))
def test_run_views_with_features(P, V, D, M, seed, scale_mult, C, eta_rec, kind, extras, gpu_device):
    """The first call of a SyncFreeBatch (synchronous route) and the second and third (pooled route, the same pool): maps and gradients at the
    bar; accumulate=False with grad_chunks=3 and a recording on_chunk, then accumulate=True on top of it (twice the gradient)."""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    fref = feature_reference(P, V, D, M, seed, scale_mult, C)
    combo = FFULL if extras else "colour+features"
    exp = expectation_f(fref, combo)
    L, flat, settings, colors, up, F = _batch_setup(fref, gpu_device)
    batch = SyncFreeBatch(granule=256, deterministic=True, **(dict(split=True, streams=4) if (extras and kind == "view") else {}))
    kw = dict(features=F, **(dict(return_alpha=True, return_depth=True) if extras else {}))
    f = upstream_of(up, C, extras)
    # call 1: no bound yet -- synchronous frames, the one-view backward with grad_out_features
    flat.flat.fill_(float("nan"))
    out = _run(batch, L, settings, colors, kind, f, accumulate=False, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, tuple) and len(out) == (4 if extras else 2) and tuple(out[-1].shape) == (V, C, H, W) and tuple(out[0].shape) == (V, 3, H, W)
    check_fmaps(out[-1], fref, "first call")
    check(*_grads(L, batch, fref, F), exp, f"run_views first call [{kind}]")
    assert batch.capacity() is not None
    # call 2: the pooled route, stored, three ranges
    calls = []
    flat.flat.fill_(float("nan")); F.grad.fill_(float("nan"))
    out = _run(batch, L, settings, colors, kind, f, accumulate=False, grad_chunks=3, on_chunk=lambda first, count: calls.append((first, count)), **kw)
    torch.cuda.synchronize()
    pool = batch._pool
    assert batch.rejected == 0 and pool is not None and out[-1].data_ptr() == pool["features"].data_ptr()
    assert pool["key"][-1] == C and pool["key"][-2] == ((("alpha", "depth") if extras else ()) + ("features",))
    assert tuple(pool["fscratch"].shape) == (V, batch.capacity() * C)
    chunks = max(1, min(3, (P + 255) // 256))
    per = ((P + chunks - 1) // chunks + 255) // 256 * 256
    assert calls == [(first, min(per, P - first)) for first in range(0, P, per)]
    check_fmaps(out[-1], fref, "second call")
    if extras:
        check_maps(out[1], out[2], fref["base"], "second call")
    for v in range(V):
        assert util.rel_l2(out[0][v].cpu().numpy(), fref["base"]["images"][v]) <= util.REL_TOL
    check(*_grads(L, batch, fref, F), exp, f"run_views pooled [{kind}]")
    stored, storedF = flat.flat.clone(), F.grad.clone()
    # call 3: the pooled route again (the same pool and buffers), added to what call 2 stored
    out3 = _run(batch, L, settings, colors, kind, f, accumulate=True, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == 0 and batch._pool is pool and out3[-1].data_ptr() == out[-1].data_ptr() and out3[0].data_ptr() == out[0].data_ptr()
    assert util.rel_l2(flat.flat.cpu().numpy(), 2.0 * stored.double().cpu().numpy()) <= 1e-6
    assert util.rel_l2(F.grad.cpu().numpy(), 2.0 * storedF.double().cpu().numpy()) <= 1e-6
    check(*_grads(L, batch, fref, F), exp, f"run_views pooled, accumulate [{kind}]", scale=2.0)


# ---- 3. forced re-rendering ----
@pytest.mark.parametrize("kind", ["batch", "view"])
def test_rejected_frames_are_rendered_again_with_their_feature_maps(kind, gpu_device):
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, C, _eta = FSCENES[2]
    fref = feature_reference(P, V, D, M, seed, scale_mult, C)
    exp = expectation_f(fref, FFULL)
    L, flat, settings, colors, up, F = _batch_setup(fref, gpu_device)
    batch = SyncFreeBatch(granule=64, deterministic=True)
    kw = dict(return_alpha=True, return_depth=True, features=F)
    flat.zero_(); F.grad.zero_()
    _run(batch, L, settings, colors, kind, upstream_of(up, C, True), **kw)                # the learning batch
    assert batch.capacity() is not None and batch.rejected == 0
    assert min(fref["base"]["counts"]) > 4 * 64
    batch.bound = 1                                         # capacity 64: below every view's instance count
    seen = []

    def upstream(v, images, alpha, depth, fmap):
        seen.append(fmap.detach().clone())
        return upstream_of(up, C, True)(v, images, alpha, depth, fmap)

    flat.flat.fill_(float("nan")); F.grad.fill_(float("nan"))
    images, alpha, depth, fmap = _run(batch, L, settings, colors, kind, upstream, accumulate=False, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == V
    # the rejected frames rendered zero maps; the second round of upstream calls saw the corrected ones
    assert bool((seen[0] == 0).all()) and len(seen) == (2 if kind == "batch" else 2 * V)
    if kind == "batch":
        check_fmaps(seen[1], fref, "the second upstream call")
    else:
        for v in range(V):
            e = util.rel_l2(seen[V + v].cpu().numpy(), fref["fmaps"][v])
            assert e <= util.tolerance("color", None), (v, e)
    check_fmaps(fmap, fref, "re-rendered")                  # in the returned (pooled) buffers
    check_maps(alpha, depth, fref["base"], "re-rendered")
    assert fmap.data_ptr() == batch._pool["features"].data_ptr()
    check(*_grads(L, batch, fref, F), exp, f"run_views re-rendered [{kind}]")
    # the bound has been learned again: the next call is sync-free and complete
    flat.flat.fill_(float("nan")); F.grad.fill_(float("nan"))
    _run(batch, L, settings, colors, kind, upstream_of(up, C, True), accumulate=False, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == V
    check(*_grads(L, batch, fref, F), exp, f"run_views after re-rendering [{kind}]")


# ---- 4. absent gradients ----
def _third_call(fref, dev, kind, upstream, requires_grad=True, accumulate=False, fill=float("nan"), **kw):
    """the third call (pooled route) of a fresh deterministic SyncFreeBatch: the flat parameter gradients, dL_dmeans2D, the batch and the features"""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    L, flat, settings, colors, up, F = _batch_setup(fref, dev, requires_grad)
    batch = SyncFreeBatch(granule=256, deterministic=True)
    if kw.pop("with_features", True):
        kw["features"] = F
    for _ in range(3):
        flat.flat.fill_(0.0 if accumulate else float("nan"))
        if requires_grad:
            F.grad.fill_(fill)
        _run(batch, L, settings, colors, kind, upstream(up), accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    assert batch.rejected == 0
    return flat.flat.clone(), batch.viewspace_grads.clone(), batch, F, L


@pytest.mark.parametrize("kind", ["batch", "view"])
def test_absent_feature_gradients_change_nothing(kind, gpu_device):
    P, V, D, M, seed, scale_mult, C, _eta = FSCENES[2]
    fref = feature_reference(P, V, D, M, seed, scale_mult, C)
    pick = lambda t, v: t if v is None else t[v]
    plain = lambda up: (lambda v, images: pick(up["dL"], v))
    unused = lambda up: (lambda v, images, fmap: (pick(up["dL"], v), None))
    g0, m0, batch0, _F, _L = _third_call(fref, gpu_device, kind, plain, with_features=False)
    assert "features" not in batch0._pool and "farr" not in batch0._pool and len(batch0._pool["key"]) == 8
    # the map returned and not used: the bits of the call without features; store mode zeroes features.grad, no scratch is allocated
    g, m, batch, F, _L = _third_call(fref, gpu_device, kind, unused)
    assert torch.equal(g, g0) and torch.equal(m, m0) and bool((F.grad == 0).all()) and batch._pool["fscratch"] is None
    # ... and accumulate leaves it as it was
    ga0, ma0, _b, _F, _L = _third_call(fref, gpu_device, kind, plain, accumulate=True, with_features=False)
    g, m, _b, F, _L = _third_call(fref, gpu_device, kind, unused, accumulate=True, fill=0.25)
    assert torch.equal(g, ga0) and torch.equal(m, ma0) and bool((F.grad == 0.25).all())
    # features that need no gradient: .grad stays None, the through-alpha share still reaches the parameters
    full = lambda up: upstream_of(up, C, False)
    g, m, batch, F, L = _third_call(fref, gpu_device, kind, full, requires_grad=False)
    assert F.grad is None and not torch.equal(g, g0)
    check(*_grads(L, batch, fref, F), expectation_f(fref, "colour+features", with_dF=False), f"features without a gradient [{kind}]")
    # a feature gradient in the even views only (the view callable: its tuple is per view)
    if kind == "view":
        even = list(range(0, V, 2))
        g, m, batch, F, L = _third_call(fref, gpu_device, kind, lambda up: upstream_of(up, C, False, fviews=even))
        check(*_grads(L, batch, fref, F), expectation_f(fref, "colour+features", fviews=even), "even views")
    else:
        # a [C,H,W] gradient from the batch callable is shared by all views
        shared = lambda up: (lambda v, images, fmap: (up["dL"], up["gF"][0]))
        expanded = lambda up: (lambda v, images, fmap: (up["dL"], up["gF"][:1].expand(V, C, H, W)))
        gs, ms, _b, Fs, _L = _third_call(fref, gpu_device, kind, shared)
        ge, me, _b, Fe, _L = _third_call(fref, gpu_device, kind, expanded)
        assert torch.equal(gs, ge) and torch.equal(ms, me) and torch.equal(Fs.grad, Fe.grad) and not torch.equal(gs, g0)


# ---- 5. wrong features ----
def test_wrong_features_raise_and_leave_the_batch_usable(gpu_device):
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, C, _eta = FSCENES[1]
    fref = feature_reference(P, V, D, M, seed, scale_mult, C)
    L, flat, settings, colors, up, F = _batch_setup(fref, gpu_device)
    batch = SyncFreeBatch(granule=256, deterministic=True)
    f = upstream_of(up, C, False)
    no_grad = F.detach().clone().requires_grad_(True)                          # requires a gradient, has no .grad
    wrong = {"float64": F.detach().double(), "17 channels": torch.zeros((P, 17), device=gpu_device), "no channel": torch.zeros((P, 0), device=gpu_device),
             "wrong P": torch.zeros((P + 1, C), device=gpu_device), "[P]": torch.zeros((P,), device=gpu_device), "on the host": F.detach().cpu(),
             "not contiguous": torch.zeros((C, P), device=gpu_device).t(), "no .grad": no_grad, "not a leaf": no_grad * 2.0, "a list": [[0.0] * C] * P}
    for route in ("synchronous", "pooled"):
        for what, bad in wrong.items():
            with pytest.raises(RuntimeError, match="features"):
                _run(batch, L, settings, colors, "batch", f, features=bad)
        flat.flat.fill_(float("nan")); F.grad.fill_(float("nan"))
        out = _run(batch, L, settings, colors, "batch", f, accumulate=False, features=F)
        torch.cuda.synchronize()
        assert batch.capacity() is not None and batch.rejected == 0
        check_fmaps(out[-1], fref, f"after the wrong features ({route})")
        check(*_grads(L, batch, fref, F), expectation_f(fref, "colour+features"), f"after the wrong features ({route})")


# ---- 6. the example ----
def test_example_fits_feature_maps_of_several_views(gpu_device):
    """examples/fit_views_features.py at a small size: the loss falls (what the silhouette / depth example's test asks of it)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fit_views_features", os.path.join(util.ROOT, "examples", "fit_views_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    vals = mod.run(steps=40, P=400, W=64, H=48, views=6, log=lines.append)
    print("\n".join(lines))
    assert len(vals) == 41 and all(np.isfinite(vals)) and vals[-1] < vals[0]
