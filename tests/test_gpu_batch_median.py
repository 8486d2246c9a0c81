"""The median of a batch's views on the device: tgs_median_views, tgs_backward_median_views, tgs_backward_batch_median_range and
tgs_surface_votes through the _C bindings, and SyncFreeBatch.median_views / backward_median_views / surface_votes behind run_views on
every route (the first, synchronous batch; the pooled batches; a batch with rejected frames).

Yardstick (tests/test_batch_median_abi.py computes and checks it on the CPU): per view the NumPy walk of the oracle's own lists, in float32
and float64; index and depth are compared on the pixels that are not AMBIGUOUS there, by Gaussian index.  Gradient: median_depth is
piecewise constant in every alpha, so under per-view upstreams g_v = standard_normal / (H W) from PCG64(6060 + v), zeroed on the ambiguous
pixels (the expectation then comes from the reference alone),
    dL_dmeans3D = the colour term + sum_v dz_v (x) z_row(view_v),   dz_v[i] = sum over the pixels of view v whose median entry is i of g_v   (float64)
and every other gradient is the colour term alone.  Bars: the isolated share at util.REL_TOL; the whole step at the frozen bar of the
batch-extras suite, per tensor min(max(1e-4, 2 eta), 1e-3) with eta from the fp32 and fp64 expectations.  The votes: exact equality with
np.bincount.  Scenes, helpers and the colour terms are those of tests/test_gpu_batch_extras.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_batch_extras as E
from tests import util
from tests.test_batch_median_abi import yardstick
from tests.test_depth_abi import z_row
from tests.test_gpu_batch_backward import _leaves, _settings, _t

pytestmark = pytest.mark.gpu

W, H = E.W, E.H
NONE = E.SCENES[0]                                          # P1-V1: no pixel of it has a median entry
RUN = E.RUN_SCENES + [NONE]


@functools.lru_cache(maxsize=None)
def scene(P, V, D, M, seed, scale_mult):
    """-> the yardstick of the scene plus, per view, the upstream gradient g_v (zero on the ambiguous pixels) and the median's share of
    dL_dmeans3D in float64 (computed once per scene, read-only)"""
    y = yardstick(P, V, D, M, seed, scale_mult)
    gMs, shares = [], []
    for v, w in enumerate(y["views"]):
        g = (np.random.Generator(np.random.PCG64(6060 + v)).standard_normal((H, W)) / (H * W)).astype(np.float32)
        g[w["ambiguous"]] = 0.0
        idx = w["index"]
        dz = np.zeros(P, np.float64)
        np.add.at(dz, idx[idx >= 0], g[idx >= 0].astype(np.float64))
        gMs.append(g)
        shares.append(dz[:, None] * z_row(y["cams"][v].viewmatrix)[None, :])
    return dict(y, gMs=gMs, shares=shares)


def check_maps(md, mi, sc, what, views=None):
    """median_index against the yardstick on every unambiguous pixel, exactly; median_depth as tests/test_gpu_median.py holds it: 0 where
    there is no entry, the oracle's depths[index] within the colour tolerance elsewhere"""
    assert md.dtype == torch.float32 and mi.dtype == torch.int32 and tuple(md.shape) == tuple(mi.shape) == (sc["V"], 1, H, W)
    d_all, i_all = md.cpu().numpy(), mi.cpu().numpy()
    for v in (range(sc["V"]) if views is None else views):
        w, d, i = sc["views"][v], d_all[v, 0], i_all[v, 0]
        ok, has = w["ok"], i >= 0
        wrong = int((i[ok] != w["index"][ok]).sum())
        assert wrong == 0, f"{what}: view {v}: {wrong} indices differ from the yardstick"
        assert i.min() >= -1 and i.max() < sc["P"] and np.all(d[~has] == 0)
        sel = ok & has
        if sel.any():
            e = util.rel_l2(d[sel], w["depths"][w["index"][sel]])
            assert e <= util.tolerance("color", None), f"{what}: view {v}: median depth rel-L2 {e:.3e}"
        if sc["P"] == 1:
            assert not has.any()
        else:
            assert has.any()


def _setup(sc, dev):
    from youreditableavatar_amd.multiview import FlatGradients
    names = ("means3D", "opacities", "scales", "rotations") + (("shs",) if sc["M"] else ())
    L = _leaves(sc["cloud"], dev, names)
    flat = FlatGradients([L[n] for n in names])
    settings = [_settings(c, sc["D"], dev) for c in sc["cams"]]
    colors = None if sc["M"] else torch.stack([_t(util.scene_input(sc["cloud"], c, "precomp")["colors_precomp"], dev) for c in sc["cams"]])
    dL = torch.stack([_t(d, dev) for d in sc["dLs"]])
    gM = torch.stack([_t(g, dev) for g in sc["gMs"]]).reshape(-1, 1, H, W)
    return L, flat, settings, colors, dL, gM


def plain(dL):
    return lambda v, images: dL if v is None else dL[v]


def one_view_maps(sc, L, settings, colors):
    """rasterize_gaussians(..., return_median=True) of every view: the maps the batch's must equal bit for bit"""
    from diff_gaussian_rasterization import rasterize_gaussians
    e = torch.Tensor([])
    md, mi = [], []
    with torch.no_grad():
        for v in range(sc["V"]):
            out = rasterize_gaussians(L["means3D"].detach(), torch.zeros_like(L["means3D"]), L["shs"].detach() if sc["M"] else e, e if sc["M"] else colors[v],
                                      L["opacities"].detach(), L["scales"].detach(), L["rotations"].detach(), e, settings[v], return_median=True)
            md.append(out[2]); mi.append(out[3])
    return torch.stack(md), torch.stack(mi)


def check_step(L, batch, ref, sc, what, scale=1.0, part=None):
    """every parameter gradient after run_views + backward_median_views at the frozen bar, as E.check applies it: the colour term, plus the
    median's share of the views ``part`` (default: all) on dL_dmeans3D only; ``scale``: the summed gradients hold that multiple of it"""
    exp = E.expectation(ref, "colour")
    (s32, v32), (s64, v64) = exp["f32"], exp["f64"]
    total = sum(sc["shares"][v] for v in (range(sc["V"]) if part is None else part))
    s32, s64 = dict(s32, dL_dmeans3D=s32["dL_dmeans3D"] + total), dict(s64, dL_dmeans3D=s64["dL_dmeans3D"] + total)
    got_sums, got_views = E._grads(L, batch, ref)
    worst = 0.0
    for k, e32 in s32.items():
        b, eta = E.bar(e32, s64[k])
        e = util.rel_l2(np.asarray(got_sums[k], np.float64).reshape(e32.shape) / scale, e32)
        print(f"{what} {k}: rel-L2 {e:.3e} (bar {b:.2e}, eta {eta:.2e})")
        assert e <= b, f"{what}: {k} rel-L2 {e:.3e} > {b:.2e}"
        worst = max(worst, e)
    for v, (one32, one64) in enumerate(zip(v32, v64)):
        for k, e32 in one32.items():
            b, eta = E.bar(e32, one64[k])
            a = np.asarray(got_views[v][k], np.float64).reshape(len(e32), -1)
            if k == "dL_dmeans2D":
                assert np.all(a[:, 2] == 0), (what, v)
                a = a[:, :e32.shape[1]] if e32.shape[1] < 3 else a
            e = util.rel_l2(a, e32)
            assert e <= b, f"{what}: view {v} {k} rel-L2 {e:.3e} > {b:.2e} (eta {eta:.2e})"
            worst = max(worst, e)
    return worst


def median_and_check(batch, sc, ones, what):
    md, mi = batch.median_views()
    torch.cuda.synchronize()
    check_maps(md, mi, sc, what)
    assert torch.equal(md, ones[0]) and torch.equal(mi, ones[1]), f"{what}: the maps differ from the one-view call's"
    return md, mi


# ---- 1. run_views, then the median and its gradient, on every route ----
@pytest.mark.parametrize("config", ["default", "split4"])
@pytest.mark.parametrize("kind", ["batch", "view"])
@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,eta_rec", RUN, ids=E.ids(RUN))
def test_median_views_and_gradient_on_every_route(P, V, D, M, seed, scale_mult, eta_rec, kind, config, gpu_device):
    """The first call of a SyncFreeBatch (synchronous frames) and the second and third (pooled frames): the maps against the yardstick and,
    bit for bit, against the one-view call; every parameter gradient of the step with backward_median_views behind it -- accumulate=False
    (with grad_chunks=3 on the pooled route), then accumulate=True on top of it (twice the gradient)."""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    sc, ref = scene(P, V, D, M, seed, scale_mult), E.reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, dL, gM = _setup(sc, gpu_device)
    ones = one_view_maps(sc, L, settings, colors)
    batch = SyncFreeBatch(granule=256, deterministic=True, **(dict(split=True, streams=4) if config == "split4" else {}))
    with pytest.raises(RuntimeError, match="run_views"):
        batch.median_views()
    rep = {}
    # call 1: no bound yet -- synchronous frames
    flat.flat.fill_(float("nan"))
    E._run(batch, ref, L, settings, colors, kind, plain(dL), accumulate=False)
    assert batch._last["pool"] is None and batch._last["sync"] == list(range(V))
    with pytest.raises(RuntimeError, match="median_views"):
        batch.backward_median_views(gM)                     # (the position maps are median_views')
    md, mi = median_and_check(batch, sc, ones, "first call")
    batch.backward_median_views(gM)
    torch.cuda.synchronize()
    rep["first"] = check_step(L, batch, ref, sc, f"first call [{kind}, {config}]")
    assert batch.capacity() is not None
    # call 2: the pooled route, stored, three ranges; the maps land in the same pooled buffers
    flat.flat.fill_(float("nan"))
    E._run(batch, ref, L, settings, colors, kind, plain(dL), accumulate=False, grad_chunks=3)
    assert batch.rejected == 0 and batch._last["sync"] == [] and len(batch._pool["key"]) == 8 and "mdz" not in batch._pool
    md2, mi2 = median_and_check(batch, sc, ones, "pooled")
    assert md2.data_ptr() == md.data_ptr() and mi2.data_ptr() == mi.data_ptr()
    batch.backward_median_views(gM if kind == "batch" else [gM[v] for v in range(V)])
    torch.cuda.synchronize()
    assert tuple(batch._pool["mdz"].shape) == (V, batch._last["cap"])
    rep["pooled"] = check_step(L, batch, ref, sc, f"pooled [{kind}, {config}]")
    stored = flat.flat.clone()
    # call 3: the pooled route again, added to what call 2 and its median pass stored
    E._run(batch, ref, L, settings, colors, kind, plain(dL), accumulate=True)
    median_and_check(batch, sc, ones, "pooled, accumulate")
    batch.backward_median_views(gM)
    torch.cuda.synchronize()
    assert batch.rejected == 0
    assert util.rel_l2(flat.flat.cpu().numpy(), 2.0 * stored.double().cpu().numpy()) <= 1e-6
    rep["accumulated"] = check_step(L, batch, ref, sc, f"pooled, accumulate [{kind}, {config}]", scale=2.0)
    util.record_parity(f"batch_median/run_views-P{P}-V{V}-M{M}-{kind}-{config}", rep)


# ---- 2. rejected frames ----
@pytest.mark.parametrize("how", ["all", "some"])
def test_rejected_frames_get_their_maps_and_their_share(how, gpu_device):
    """A batch whose bound is too small for all / for some of its views: run_views renders those again; median_views renders them once more
    (the pool does not hold their frames), the others come from the pool; a view without a gradient (None) takes no part."""
    from diff_gaussian_rasterization import _C
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, _eta = E.SCENES[2]
    sc, ref = scene(P, V, D, M, seed, scale_mult), E.reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, dL, gM = _setup(sc, gpu_device)
    ones = one_view_maps(sc, L, settings, colors)
    batch = SyncFreeBatch(granule=64, deterministic=True)
    flat.zero_()
    E._run(batch, ref, L, settings, colors, "batch", plain(dL))                 # the learning batch
    E._run(batch, ref, L, settings, colors, "batch", plain(dL))                 # a pooled batch: its Meta records name every view's count
    assert batch.capacity() is not None and batch.rejected == 0
    counts = sorted(_C.decode_meta_full(m)[0] for m in batch._pool["host"])
    assert counts[0] > 4 * 64 and counts[-1] - counts[0] > 2 * 64
    batch.bound = 1 if how == "all" else int((counts[0] + counts[-1]) / 2 / batch.headroom)      # capacity 64 / between the smallest and the largest count
    flat.flat.fill_(float("nan"))
    E._run(batch, ref, L, settings, colors, "batch", plain(dL), accumulate=False)
    redo = batch._last["sync"]
    assert batch.rejected == len(redo) and (len(redo) == V if how == "all" else 0 < len(redo) < V), redo
    median_and_check(batch, sc, ones, f"rejected ({how})")
    part = [v for v in range(V) if v != 2]
    batch.backward_median_views([gM[v] if v in part else None for v in range(V)])
    torch.cuda.synchronize()
    check_step(L, batch, ref, sc, f"rejected ({how})", part=part)
    # the bound has been learned again: the next call is sync-free and complete
    flat.flat.fill_(float("nan"))
    E._run(batch, ref, L, settings, colors, "batch", plain(dL), accumulate=False)
    assert batch.rejected == len(redo) and batch._last["sync"] == []
    median_and_check(batch, sc, ones, f"after the rejection ({how})")
    batch.backward_median_views(gM)
    torch.cuda.synchronize()
    check_step(L, batch, ref, sc, f"after the rejection ({how})")


# ---- 3. the entry points on frames from _C.forward_views ----
class Frames(E.Frames):
    def __init__(self, ref, dev):
        from diff_gaussian_rasterization import _C
        super().__init__(ref, dev)
        z = lambda dt: torch.zeros((self.V, H, W), dtype=dt, device=dev)
        self.md, self.mi, self.mp, self.marr = z(torch.float32), z(torch.int32), z(torch.int32), _C.ViewMedianArray(self.V)
        self.mdz = torch.zeros((self.V, self.cap), device=dev)
        for v in range(self.V):
            m = self.marr[v]
            m.out_depth, m.out_index, m.out_pos = self.md[v].data_ptr(), self.mi[v].data_ptr(), self.mp[v].data_ptr()

    def median(self):
        from diff_gaussian_rasterization import _C
        self.md.fill_(float("nan")); self.mi.fill_(12345); self.mp.fill_(12345)
        _C.median_views([self.stream], self.P, self.arr, self.marr, self.V)
        torch.cuda.synchronize()
        return self.md.clone(), self.mi.clone(), self.mp.clone()

    def median_gradient(self, gM, part, ranges):
        """the isolated share: k_median_bwd of the views ``part``, then the range pass into a zeroed buffer"""
        from diff_gaussian_rasterization import _C
        self.mdz.fill_(float("nan"))                        # (the call zero-fills the rows of the views that take part)
        for v in range(self.V):
            m = self.marr[v]
            m.dL_dmedian_depth = gM[v].data_ptr() if v in part else None
            m.dz_scratch = self.mdz[v].data_ptr() if v in part else None
        _C.backward_median_views([self.stream], self.P, self.arr, self.marr, self.V)
        out = torch.zeros((self.P, 3), device=self.dev)
        for first, count in ranges:
            _C.backward_batch_median_raw(self.stream, self.P, self.arr, self.marr, self.V, out.data_ptr(), first, count)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(self.mdz[v]).all()) for v in part), "dz scratch was not zero-filled"
        return out


def _ranges(P, chunks):
    n = max(1, min(chunks, (P + 255) // 256))
    per = ((P + n - 1) // n + 255) // 256 * 256
    return [(first, min(per, P - first)) for first in range(0, P, per)]


ENTRY = [E.SCENES[1], E.SCENES[2], E.SCENES[3], NONE]       # V = 9 and 17 cross BATCH_VIEWS = 8; V = 8 is exactly one launch


@pytest.mark.parametrize("P,V,D,M,seed,scale_mult,eta_rec", ENTRY, ids=E.ids(ENTRY))
def test_entry_points_on_frames_of_forward_views(P, V, D, M, seed, scale_mult, eta_rec, gpu_device):
    sc, ref = scene(P, V, D, M, seed, scale_mult), E.reference(P, V, D, M, seed, scale_mult)
    fr = Frames(ref, gpu_device)
    # the maps between forward_views and the backward ...
    md, mi, mp = fr.median()
    check_maps(md.reshape(V, 1, H, W), mi.reshape(V, 1, H, W), sc, "tgs_median_views")
    has = mi >= 0
    assert torch.equal(mp > 0, has) and bool((mp[~has] == 0).all()) and bool((md[~has] == 0).all()) and bool((mi[~has] == -1).all())
    # ... and behind the whole step: the same bits (the step's backward writes none of the arrays the pass reads)
    fr.render_backward("colour")
    fr.gauss_backward(fr.into(lambda s: torch.zeros(s, device=gpu_device)), accumulate=False)
    for a, b in zip((md, mi, mp), fr.median()):
        assert torch.equal(a, b), "the maps behind the step differ from those in front of its backward"
    # the isolated gradient: sum_v dz_v (x) z_row(view_v) in float64, at REL_TOL
    gM = torch.stack([_t(g, gpu_device) for g in sc["gMs"]])
    everyone = list(range(V))
    for part in (everyone, [v for v in everyone if v != V // 2]):
        want = sum((sc["shares"][v] for v in part), np.zeros((P, 3)))
        got = {}
        for chunks in (1, 3):
            got[chunks] = fr.median_gradient(gM, part, _ranges(P, chunks))
            e = util.rel_l2(got[chunks].cpu().numpy(), want)
            print(f"P{P}-V{V} views {len(part)} of {V}, {chunks} range(s): median share rel-L2 {e:.3e}")
            if np.any(want):
                assert e <= util.REL_TOL
            else:
                assert not bool(got[chunks].any())
        assert torch.equal(got[1], got[3]), "ranges differ from the whole launch"
        assert torch.equal(got[1], fr.median_gradient(gM, part, _ranges(P, 1))), "two runs differ"
    if not part:                                            # (V = 1 without its one view: nothing is launched, nothing is added)
        assert not bool(got[1].any())
    dead = ~(fr.buf["radii"].cpu().numpy() > 0).any(axis=0)
    assert not bool(got[1].cpu().numpy()[dead].any()), "Gaussians culled in every view must be exactly 0"


# ---- 4. nothing changes without the calls ----
def test_a_step_without_the_calls_is_the_step_of_before(gpu_device):
    """Three deterministic steps that never call the new methods, and three with median_views / backward_median_views behind the first two:
    the third step's gradients, dL_dmeans2D and images are the same bits (the calls leave the pooled frames and the pool's key alone), and
    the object that never called them holds none of their buffers."""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, _eta = E.SCENES[2]
    sc, ref = scene(P, V, D, M, seed, scale_mult), E.reference(P, V, D, M, seed, scale_mult)
    out = {}
    for with_calls in (False, True):
        L, flat, settings, colors, dL, gM = _setup(sc, gpu_device)
        batch = SyncFreeBatch(granule=256, deterministic=True)
        for step in range(3):
            flat.flat.fill_(float("nan"))
            images = E._run(batch, ref, L, settings, colors, "batch", plain(dL), accumulate=False)
            if with_calls and step < 2:
                batch.median_views()
                batch.backward_median_views(gM)
        torch.cuda.synchronize()
        assert batch.rejected == 0 and torch.is_tensor(images) and len(batch._pool["key"]) == 8
        if not with_calls:
            assert batch._mpool is None and "mdz" not in batch._pool and "marr" not in batch._pool
        out[with_calls] = (flat.flat.clone(), batch.viewspace_grads.clone(), images.clone())
        if with_calls:                                      # median_views alone writes no gradient and no image
            batch.median_views()
            torch.cuda.synchronize()
            assert torch.equal(flat.flat, out[True][0]) and torch.equal(images, out[True][2])
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


# ---- 5. surface votes ----
def _votes_reference(idx, P, mask):
    flat = idx.reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < P)
    seen = np.bincount(flat[ok], minlength=P)
    hits = None if mask is None else np.bincount(flat[ok & (mask.reshape(-1) != 0)], minlength=P)
    return seen, hits


def _check_votes(idx, P, mask, dev, what):
    from youreditableavatar_amd.multiview import surface_votes
    ti = torch.from_numpy(idx).to(dev)
    tm = None if mask is None else torch.from_numpy(mask).to(dev)
    seen, hits = surface_votes(ti, P, tm)
    want_seen, want_hits = _votes_reference(idx, P, mask)
    assert seen.dtype == torch.int32 and tuple(seen.shape) == (P,)
    assert np.array_equal(seen.cpu().numpy(), want_seen), what
    if mask is None:
        assert hits is None
    else:
        assert hits.dtype == torch.int32 and np.array_equal(hits.cpu().numpy(), want_hits), what
    again = surface_votes(ti, P, tm)
    assert torch.equal(again[0], seen) and (mask is None or torch.equal(again[1], hits)), f"{what}: two runs differ"
    return seen, hits


def test_surface_votes_equal_bincount(gpu_device):
    from youreditableavatar_amd.multiview import surface_votes
    dev = gpu_device
    rng = np.random.Generator(np.random.PCG64(77))
    shape = (3, 1, 37, 53)                                  # 5883 pixels: no multiple of 64, 23 workgroups
    n = int(np.prod(shape))
    P = 50
    # runs of equal indices, 1 .. 200 pixels long (crossing lanes, waves and workgroups), with -1, indices < -1 and >= P mixed in
    values = np.concatenate([np.arange(P), [-1, -1, -1, -7, -(1 << 31), P, P + 5, (1 << 31) - 1]])
    runs = []
    while sum(len(r) for r in runs) < n:
        runs.append(np.full(int(rng.integers(1, 201)), rng.choice(values)))
    idx = np.concatenate(runs)[:n].astype(np.int32).reshape(shape)
    assert (idx < -1).any() and (idx >= P).any() and (idx == -1).any()
    bits = rng.integers(0, 2, shape).astype(bool)
    bytes_ = np.where(bits, rng.integers(1, 256, shape), 0).astype(np.uint8)      # any non-zero byte counts
    for what, mask in (("no mask", None), ("bool mask", bits), ("uint8 mask", bytes_)):
        _check_votes(idx, P, mask, dev, f"runs, {what}")
    # one index per pixel, shuffled: no two neighbours equal (every lane is a head)
    _check_votes(rng.permutation(n).astype(np.int32).reshape(shape), n, bits, dev, "every pixel its own index")
    # runs that end exactly at wave boundaries, and one run over everything
    _check_votes((np.arange(n) // 64 % 7).astype(np.int32).reshape(shape), 7, bits, dev, "runs of 64")
    _check_votes(np.full(shape, -1, np.int32), P, bits, dev, "all -1")
    seen, hits = _check_votes(np.full(shape, 17, np.int32), P, bits, dev, "all one index")
    assert int(seen[17]) == n and int(seen.sum()) == n and int(hits[17]) == int(bits.sum())
    _check_votes(rng.choice(np.array([0, 0, 0, -1, 1], np.int32), shape).astype(np.int32), 1, bytes_, dev, "P = 1")
    _check_votes(idx[0], P, bits[0], dev, "[1,H,W]")
    # out= accumulates: two chunks of views into the same counters equal one call over all of them; without masks hits stays untouched
    ti, tm = torch.from_numpy(idx).to(dev), torch.from_numpy(bits).to(dev)
    whole = surface_votes(ti, P, tm)
    acc = (torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))
    got = surface_votes(ti[:2], P, tm[:2], out=acc)
    assert got[0] is acc[0] and got[1] is acc[1]
    surface_votes(ti[2:], P, tm[2:], out=acc)
    assert torch.equal(acc[0], whole[0]) and torch.equal(acc[1], whole[1])
    seen2, none = surface_votes(ti, P, out=(acc[0], None))
    assert none is None and torch.equal(seen2, 2 * whole[0]) and torch.equal(acc[1], whole[1])
    for bad in ((acc[0].long(), acc[1]), (acc[0][:-1], acc[1]), (acc[0], None)):
        with pytest.raises(RuntimeError, match="out"):
            surface_votes(ti, P, tm, out=bad)
    # an empty model
    seen0, hits0 = surface_votes(torch.full((1, 1, 4, 4), -1, dtype=torch.int32, device=dev), 0, torch.ones((1, 1, 4, 4), dtype=torch.bool, device=dev))
    assert tuple(seen0.shape) == (0,) and tuple(hits0.shape) == (0,)


def test_surface_votes_on_the_maps_of_a_batch(gpu_device):
    """the real maps of P2000-V8 (up to hundreds of pixels share a surface splat) with a rectangle mask per view"""
    from youreditableavatar_amd.multiview import SyncFreeBatch
    P, V, D, M, seed, scale_mult, _eta = E.SCENES[2]
    sc, ref = scene(P, V, D, M, seed, scale_mult), E.reference(P, V, D, M, seed, scale_mult)
    L, flat, settings, colors, dL, _gM = _setup(sc, gpu_device)
    batch = SyncFreeBatch(granule=256, deterministic=True)
    for _ in range(2):                                      # (the second call's frames are the pool's)
        E._run(batch, ref, L, settings, colors, "batch", plain(dL), accumulate=False)
    _md, mi = batch.median_views()
    masks = np.zeros((V, 1, H, W), bool)
    for v in range(V):
        masks[v, :, 10 + 3 * v:70 + 3 * v, 20 + 7 * v:120 + 7 * v] = True
    idx = mi.cpu().numpy()
    seen, hits = _check_votes(idx, P, masks, gpu_device, "P2000-V8")
    assert int(seen.sum()) == int((idx >= 0).sum()) > 8 * 2000 and 0 < int(hits.sum()) < int(seen.sum())
    assert int(seen.max()) > 64                             # a splat that is the surface of more pixels than a wave has lanes


# ---- 6. the example ----
def test_example_lifts_masks_and_fits_median_depths_of_several_views(gpu_device):
    """examples/lift_masks_views.py at a small size: Gaussians are picked under the masks and the loss falls."""
    spec = importlib.util.spec_from_file_location("lift_masks_views", os.path.join(util.ROOT, "examples", "lift_masks_views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    n_picked, vals = mod.run(steps=40, P=400, W=64, H=48, views=4, log=lines.append)
    print("\n".join(lines))
    assert n_picked > 0 and len(vals) == 41 and all(np.isfinite(vals)) and vals[-1] < vals[0]
