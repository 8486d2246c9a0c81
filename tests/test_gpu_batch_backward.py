"""The batched per-Gaussian backward (tgs_backward_batch: k_preprocess_bwd_batch / k_preprocess_bwd_batch_split) in every mode of its dispatch,
against the CPU oracle in double and against the per-view HIP path.

launch_preprocess_bwd_batch picks one of six kernels:

    colour \\ covariance      scale + rotation        cov3D_precomp
    SH, M == 16               split<true>            split<false>
    SH, M in {1, 4, 9}        batch<true, true>      batch<true, false>
    colors_precomp            batch<false, true>     batch<false, false>

Every case renders V views with _C.rasterize_gaussians, runs the per-pixel half of each view's backward (_C.rasterize_gaussians_backward_render,
an upstream gradient of its own per view) and then ONE _C.rasterize_gaussians_backward_batch, and checks
  (a) every parameter gradient and every view's dL_dmeans2D (dL_dcolors) against the sum over the views of the oracle built in double
      (the reference's function in exact arithmetic).  The bar is the frozen one, min(max(1e-4, 2 eta), 1e-3), with eta = rel_l2(sum of the fp32
      oracle, sum of the double oracle) of the same tensor; the scenes were screened on the CPU oracle so that 2 eta <= 1e-4 everywhere (the
      plain 1e-4 bar), with the oracle's cut-off variants (f32_in / f32_out) as quiet as the plain fp32 build.  The largest eta of the case is
      recorded in its parameters; a scene whose eta grows past 1.5 x that no longer means what it was chosen for and fails.
  (b) against the per-view HIP path (_C.rasterize_gaussians_backward, deterministic), summed: whole tensors within 2e-5, every row within
      1e-3 of its own size (plus 1e-3 of the rms row), the per-view dL_dmeans2D (and dL_dcolors) bit for bit -- both evaluate the same tile
      partials in the same order (slab_sum).
  (c) exact properties: store mode writes every element (nothing is left of a NaN-filled buffer; Gaussians culled in every view, SH
      coefficients above the active degree and dL_dmeans2D[:, 2] are exactly 0), accumulate mode adds the store result to what the buffers hold.
The active SH degree D is set below the stored one (M = (deg + 1)^2) in most cases: the trainers' sh_levels schedule renders at degree 0 for
most of its iterations.  V in {1, 8, 9, 17} crosses the launch's BATCH_VIEWS = 8 (a later chunk adds to what the first stored); P sits at the
ragged tail of a 128-Gaussian (split) or 256-Gaussian (one-thread) workgroup; some cases mix image sizes and fields of view in one batch.
"""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

REL_TOL = util.REL_TOL          # 1e-4: min(max(1e-4, 2 eta), 1e-3) with 2 eta <= 1e-4 (screened)
PER_VIEW_TOL = 2e-5             # against the per-view HIP path, whole tensors (tests/test_gpu_api.py::test_batched_backward_equals_per_view_backward)
ROW_TOL = 1e-3                  # ... and row by row
SIZES = ((176, 112, 45.0), (130, 97, 38.0), (200, 150, 52.0))     # (W, H, vertical field of view): mixed batches cycle through them
DEG = {1: 0, 4: 1, 9: 2, 16: 3}
FAR = (0.0, 40.0, 0.0)          # every 97th Gaussian of a scene is moved here: off screen in every view (radii 0 everywhere)

# (kernel, P, V, D, M, mixed views, cloud seed, scale_mult, recorded eta).  M = 0: colors_precomp.  eta: the largest rel_l2(sum fp32 oracle,
# sum double oracle) over the compared tensors of the case (parameter gradients and every view's dL_dmeans2D / dL_dcolors), from the screen.
CASES = [
    ("split_sr", 1, 1, 0, 16, False, 3, 0.2, 9.3e-7),
    ("split_sr", 129, 9, 1, 16, False, 4, 1.0, 9.9e-6),
    ("split_sr", 3001, 17, 2, 16, True, 705, 2.0, 1.6e-5),
    ("split_sr", 2000, 8, 3, 16, False, 1406, 2.0, 1.1e-5),
    ("split_cov", 1, 9, 0, 16, False, 7, 0.2, 9.6e-6),
    ("split_cov", 129, 17, 3, 16, True, 108, 1.0, 5.7e-6),
    ("split_cov", 2003, 8, 1, 16, False, 509, 2.0, 5.9e-6),
    ("batch_sh_sr", 1, 8, 2, 9, False, 10, 0.2, 2.4e-6),
    ("batch_sh_sr", 257, 17, 0, 9, True, 811, 1.0, 8.4e-6),
    ("batch_sh_sr", 2999, 9, 1, 4, False, 512, 2.0, 4.6e-6),
    ("batch_sh_cov", 257, 1, 0, 1, False, 113, 1.0, 3.3e-6),
    ("batch_sh_cov", 3001, 9, 2, 9, True, 1114, 2.0, 4.6e-6),
    ("batch_col_sr", 1, 17, 0, 0, False, 115, 0.2, 1.8e-6),
    ("batch_col_sr", 2999, 8, 0, 0, True, 616, 2.0, 5.9e-6),
    ("batch_col_cov", 257, 9, 0, 0, True, 17, 1.0, 4.2e-6),
    ("batch_col_cov", 3001, 1, 0, 0, False, 118, 2.0, 4.3e-6),
]
CASE_IDS = [f"{k}-P{P}-V{V}-D{D}-M{M}{'-mixed' if mix else ''}" for k, P, V, D, M, mix, *_ in CASES]


def make_scene(P, V, D, M, mixed, seed, scale_mult, cov3d):
    """-> (cloud, cams, upstream gradients).  M = 0: colours precomputed per view from degree-3 SH."""
    from youreditableavatar_amd import scenes
    cloud = scenes.make_cloud(P, DEG[M] if M else 3, seed=seed, scale_mult=scale_mult)
    cloud["sh_degree"] = D if M else 3
    if P >= 97:
        cloud["means3D"][::97] = np.asarray(FAR, np.float32)
    if cov3d:
        from oracle.emu_crosscheck_cov import cov3d_from
        cloud["cov3D_precomp"] = cov3d_from(cloud["scales"], cloud["rotations"])
    cams, dLs = [], []
    for v, az in enumerate(np.linspace(0.0, 360.0, V, endpoint=False) + 7.0 * seed):
        W, H, fov = SIZES[v % len(SIZES)] if mixed else SIZES[0]
        cams.append(scenes.orbit_camera(W, H, azimuth_deg=float(az), fovy_deg=fov))
        dLs.append(scenes.upstream_gradient(W, H, seed=1000 * seed + v))
    return cloud, cams, dLs


def _keys(M, cov3d):
    params = ["dL_dmeans3D", "dL_dopacity"] + (["dL_dsh"] if M else []) + (["dL_dcov3D"] if cov3d else ["dL_dscales", "dL_drotations"])
    return params, ["dL_dmeans2D"] + ([] if M else ["dL_dcolors"])


def oracle_sums(cloud, cams, dLs, M, cov3d, variant):
    """-> (per-view oracle results, {parameter gradient: sum over the views in float64})"""
    params, _ = _keys(M, cov3d)
    per_view, sums = [], {}
    for cam, dL in zip(cams, dLs):
        ref = util.oracle_run(util.scene_input(cloud, cam, "sh" if M else "precomp", "cov3d" if cov3d else "scale_rot"), dL, variant=variant)
        per_view.append(ref)
        for k in params:
            sums[k] = sums.get(k, 0.0) + np.asarray(ref[k], np.float64)
    return per_view, sums


def scene_eta(cloud, cams, dLs, M, cov3d, variants=("f32",)):
    """the largest rel_l2(fp32 oracle, double oracle) over the summed parameter gradients and the per-view gradients; -> (eta, double results)"""
    params, views = _keys(M, cov3d)
    f64_views, f64 = oracle_sums(cloud, cams, dLs, M, cov3d, "f64")
    eta = 0.0
    for variant in variants:
        f32_views, f32 = oracle_sums(cloud, cams, dLs, M, cov3d, variant)
        eta = max([eta] + [util.rel_l2(f32[k], f64[k]) for k in params] +
                  [util.rel_l2(a[k], b[k]) for a, b in zip(f32_views, f64_views) for k in views] +
                  [util.rel_l2(a["color"], b["color"]) for a, b in zip(f32_views, f64_views)])
    return eta, f64_views, f64


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


class HipScene:
    """The scene on the device: parameters, and per view its settings, upstream gradient and (colors_precomp) colours."""

    def __init__(self, cloud, cams, dLs, M, cov3d, dev):
        self.dev, self.M, self.cov3d, self.P = dev, M, cov3d, cloud["means3D"].shape[0]
        self.D = int(cloud["sh_degree"])
        e = torch.Tensor([])
        self.means, self.opac = _t(cloud["means3D"], dev), _t(cloud["opacities"], dev)
        self.shs = _t(cloud["shs"], dev) if M else e
        self.scales, self.rots = (e, e) if cov3d else (_t(cloud["scales"], dev), _t(cloud["rotations"], dev))
        self.cov = _t(cloud["cov3D_precomp"], dev) if cov3d else e
        self.cams, self.dLs = cams, [_t(d, dev) for d in dLs]
        self.colors = [_t(util.scene_input(cloud, c, "precomp")["colors_precomp"], dev) if not M else e for c in cams]

    def forward(self, v, **kw):
        c = self.cams[v]
        from diff_gaussian_rasterization import _C
        bg, vm, pm, cp = _t(c.bg, self.dev), _t(c.viewmatrix, self.dev), _t(c.projmatrix, self.dev), _t(c.campos, self.dev)
        out = _C.rasterize_gaussians(bg, self.means, self.colors[v], self.opac, self.scales, self.rots, 1.0, self.cov, vm, pm, c.tanfovx, c.tanfovy,
                                     c.image_height, c.image_width, self.shs, self.D, cp, False, False, **kw)
        R, color, radii, geom, binning, img = out[:6]
        return dict(viewmatrix=vm, projmatrix=pm, campos=cp, bg=bg, tanfovx=c.tanfovx, tanfovy=c.tanfovy, image_height=c.image_height,
                    image_width=c.image_width, radii=radii, geom=geom, binning=binning, img=img, R=R, color=color)

    def per_view_backward(self, v):
        """_C.rasterize_gaussians_backward of view v on a state of its own -> {tensor: [P, ...]} on the device"""
        from diff_gaussian_rasterization import _C
        s, c = self.forward(v), self.cams[v]
        g = _C.rasterize_gaussians_backward(s["bg"], self.means, s["radii"], self.colors[v], self.scales, self.rots, 1.0, self.cov, s["viewmatrix"],
                                            s["projmatrix"], c.tanfovx, c.tanfovy, self.dLs[v], self.shs, self.D, s["campos"], s["geom"], s["R"],
                                            s["binning"], s["img"], False)
        return dict(zip(("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"), g))

    def rendered(self, v):
        """forward + the per-pixel half of the backward: a view ready for the batch pass"""
        from diff_gaussian_rasterization import _C
        s = self.forward(v)
        _C.rasterize_gaussians_backward_render(s["bg"], self.dLs[v], s["R"], s["binning"], s["img"], self.P)
        return s

    def into(self, fill):
        P, dev = self.P, self.dev
        shapes = dict(means3D=(P, 3), opacities=(P, 1))
        if self.M:
            shapes["sh"] = (P, self.M, 3)
        shapes.update(dict(cov3D_precomp=(P, 6)) if self.cov3d else dict(scales=(P, 3), rotations=(P, 4)))
        return {k: fill(s) for k, s in shapes.items()}

    def batch(self, views, into, accumulate):
        from diff_gaussian_rasterization import _C
        return _C.rasterize_gaussians_backward_batch(views, self.means, self.shs if self.M else None, self.D, self.scales if not self.cov3d else None,
                                                     self.rots if not self.cov3d else None, 1.0, self.cov if self.cov3d else None, into, accumulate=accumulate)


INTO = {"dL_dmeans3D": "means3D", "dL_dopacity": "opacities", "dL_dsh": "sh", "dL_dscales": "scales", "dL_drotations": "rotations", "dL_dcov3D": "cov3D_precomp"}


def worst_row(x, ref) -> float:
    """max over the rows p of |x_p - ref_p| / (|ref_p| + 1e-3 rms(|ref|)): an error confined to a few rows (one workgroup's tail, one
    chunk, one view) that a whole-tensor norm averages away"""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    rn = np.linalg.norm(ref, axis=1)
    floor = 1e-3 * float(np.sqrt(np.mean(rn * rn)))
    d = np.linalg.norm(x - ref, axis=1)
    if floor == 0.0:
        return float(d.max()) if d.size else 0.0
    return float((d / (rn + floor)).max())


@pytest.mark.parametrize("kernel,P,V,D,M,mixed,seed,scale_mult,eta_rec", CASES, ids=CASE_IDS)
def test_batch_backward_matrix(kernel, P, V, D, M, mixed, seed, scale_mult, eta_rec, gpu_device):
    """One cell of the dispatch table through the ABI: (a) against the double oracle, (b) against the per-view HIP path, (c) store /
    accumulate properties -- see the module docstring."""
    from diff_gaussian_rasterization import _C
    cov3d = kernel.endswith("cov")
    params, view_keys = _keys(M, cov3d)
    cloud, cams, dLs = make_scene(P, V, D, M, mixed, seed, scale_mult, cov3d)
    eta, f64_views, f64 = scene_eta(cloud, cams, dLs, M, cov3d)
    assert eta <= 1.5 * eta_rec, f"the scene's own fp32 noise grew: eta {eta:.3g} > 1.5 x {eta_rec:.3g}"
    assert 2.0 * eta <= REL_TOL
    hs = HipScene(cloud, cams, dLs, M, cov3d, gpu_device)
    rep = {"eta": eta}
    _C.set_deterministic(True)
    try:
        # the per-view HIP path, summed over the views in double
        pv = [hs.per_view_backward(v) for v in range(V)]
        pv_sum = {k: sum(g[k].double().cpu().numpy() for g in pv) for k in params}
        views = [hs.rendered(v) for v in range(V)]
        radii = np.stack([s["radii"].cpu().numpy() for s in views])
        dead = ~(radii > 0).any(axis=0)
        if P >= 97:
            assert dead[::97].all() and dead.sum() < P // 2       # the scene has Gaussians culled in every view, and not too many
        # store mode: NaN-filled buffers, every element written
        got = hs.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
        outs = hs.batch(views, got, accumulate=False)
        torch.cuda.synchronize()
        g = {k: got[INTO[k]].cpu().numpy() for k in params}
        per_view = [{"dL_dmeans2D": a.cpu().numpy(), **({} if M else {"dL_dcolors": b.cpu().numpy()})} for a, b in outs]
        for k in params:
            assert np.isfinite(g[k]).all(), f"{k}: store mode left elements unwritten"
            assert np.all(g[k][dead] == 0), f"{k}: Gaussians culled in every view must be exactly 0"
        for v, d in enumerate(per_view):
            for k in view_keys:
                assert np.isfinite(d[k]).all() and np.all(d[k][~(radii[v] > 0)] == 0), (v, k)
            assert np.all(d["dL_dmeans2D"][:, 2] == 0), v
        if M:
            live = (D + 1) ** 2
            assert np.all(g["dL_dsh"][:, live:] == 0), "SH coefficients above the active degree must be exactly 0"
            assert np.any(g["dL_dsh"][:, :live] != 0)
        # (a) against the oracle in double
        for k in params:
            e = rep[k] = util.rel_l2(g[k], f64[k])
            assert e <= REL_TOL, f"{k}: rel-L2 to the double oracle {e:.3e} > {REL_TOL:.0e}"
        for v, d in enumerate(per_view):
            for k in view_keys:
                e = util.rel_l2(d[k], f64_views[v][k])
                rep[k] = max(rep.get(k, 0.0), e)
                assert e <= REL_TOL, f"view {v} {k}: rel-L2 to the double oracle {e:.3e} > {REL_TOL:.0e}"
        # (b) against the per-view HIP path
        for k in params:
            e = rep[k + "|per_view"] = util.rel_l2(g[k], pv_sum[k])
            assert e <= PER_VIEW_TOL, f"{k}: rel-L2 to the per-view path {e:.3e} > {PER_VIEW_TOL:.0e}"
            r = rep[k + "|row"] = worst_row(g[k], pv_sum[k])
            assert r <= ROW_TOL, f"{k}: worst row against the per-view path {r:.3e} (row {int(np.argmax(np.linalg.norm(g[k].reshape(P, -1) - pv_sum[k].reshape(P, -1), axis=1)))})"
        for v, (a, b) in enumerate(outs):
            rep["dL_dmeans2D|per_view"] = max(rep.get("dL_dmeans2D|per_view", 0.0), util.rel_l2(a.cpu().numpy(), pv[v]["dL_dmeans2D"].cpu().numpy()))
            assert torch.equal(a, pv[v]["dL_dmeans2D"]), f"view {v}: dL_dmeans2D differs from the per-view path"
            if not M:
                assert torch.equal(b, pv[v]["dL_dcolors"]), f"view {v}: dL_dcolors differs from the per-view path"
        # (c) accumulate adds the store result to what the buffers hold
        gen = torch.Generator(device=gpu_device).manual_seed(seed)
        base = hs.into(lambda s: torch.randn(s, device=gpu_device, generator=gen) * 1e-3)
        acc = {k: b.clone() for k, b in base.items()}
        hs.batch(views, acc, accumulate=True)
        for k in params:
            n = INTO[k]
            assert util.rel_l2(acc[n].cpu().numpy(), (base[n] + got[n]).cpu().numpy()) <= 1e-6, k
    finally:
        _C.set_deterministic(False)
    util.record_parity(f"batch_backward/{kernel}-P{P}-V{V}-D{D}-M{M}", rep)


@pytest.mark.parametrize("M", [16, 9])
def test_rejected_view_contributes_nothing(M, gpu_device):
    """A frame the sync-free forward (tgs_forward_async, the path of rasterize_accumulate(r_capacity=...)) could not fit is rejected on the
    device: its dL_dmeans2D is all zero and, inside one 8-view chunk, the parameter gradients are bit for bit those of the batch without it."""
    from diff_gaussian_rasterization import _C
    cloud, cams, dLs = make_scene(2000, 8, 1, M, False, 21, 2.0, False)
    hs = HipScene(cloud, cams, dLs, M, False, gpu_device)
    views = [hs.rendered(v) for v in range(8)]
    bad = hs.forward(3, r_capacity=16)
    assert _C.frame_status(bad["img"])[1] & _C.FRAME_REJECTED
    _C.rasterize_gaussians_backward_render(bad["bg"], hs.dLs[3], bad["R"], bad["binning"], bad["img"], hs.P)
    with_bad = views[:3] + [bad] + views[4:]
    without = views[:3] + views[4:]
    a = hs.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
    b = hs.into(lambda s: torch.full(s, float("nan"), device=gpu_device))
    outs_a = hs.batch(with_bad, a, accumulate=False)
    outs_b = hs.batch(without, b, accumulate=False)
    assert torch.all(outs_a[3][0] == 0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(outs_a[:3] + outs_a[4:], outs_b):
        assert torch.equal(x[0], y[0])
    assert float(a["means3D"].abs().max()) > 0


def _view_array(views, P, dev, fill):
    """a tgs_view_t array for _C.backward_batch_raw; the per-view dL_dmeans2D outputs are filled with ``fill``"""
    from diff_gaussian_rasterization import _C
    arr = _C.ViewArray(len(views))
    g2d = []
    for i, v in enumerate(views):
        g = torch.full((P, 3), fill, device=dev)
        a = arr[i]
        a.width, a.height, a.tan_fovx, a.tan_fovy = int(v["image_width"]), int(v["image_height"]), float(v["tanfovx"]), float(v["tanfovy"])
        a.viewmatrix, a.projmatrix, a.campos, a.radii = v["viewmatrix"].data_ptr(), v["projmatrix"].data_ptr(), v["campos"].data_ptr(), v["radii"].data_ptr()
        a.geom_buffer, a.binning_buffer, a.img_buffer, a.R = v["geom"].data_ptr(), v["binning"].data_ptr(), v["img"].data_ptr(), int(v["R"])
        a.dL_dmean2D, a.dL_dcolor = g.data_ptr(), None
        g2d.append(g)
    return arr, g2d


CANARY = -7.75


@pytest.mark.parametrize("M", [16, 9])
def test_batch_ranges_leave_the_rest_untouched(M, gpu_device):
    """tgs_backward_batch_range (scale + rotation path): ranges [first, first + count) on multiples of 256, the last one ending at a ragged P.
    Outside each range every output (parameter gradients and every view's dL_dmeans2D) stays bit for bit what it was; inside, and as the
    union of the ranges, the result is bit for bit the whole launch -- stored, and added to a non-zero buffer."""
    from diff_gaussian_rasterization import _C
    P, V, D = 1800, 9, 1
    cloud, cams, dLs = make_scene(P, V, D, M, False, 31, 2.0, False)
    hs = HipScene(cloud, cams, dLs, M, False, gpu_device)
    views = [hs.rendered(v) for v in range(V)]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    ranges = [(0, 256), (256, 768), (1024, P - 1024)]
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    start = {False: lambda s: torch.full(s, CANARY, device=gpu_device), True: lambda s: torch.randn(s, device=gpu_device, generator=gen)}

    def launch(bufs, g2d_fill, accumulate, first=0, count=None):
        arr, g2d = _view_array(views, P, gpu_device, g2d_fill)
        _C.backward_batch_raw(stream, P, D, M, arr, V, hs.means.data_ptr(), hs.shs.data_ptr(), hs.scales.data_ptr(), 1.0, hs.rots.data_ptr(),
                              bufs["opacities"].data_ptr(), bufs["means3D"].data_ptr(), bufs["sh"].data_ptr(), bufs["scales"].data_ptr(),
                              bufs["rotations"].data_ptr(), accumulate, first=first, count=count)
        torch.cuda.synchronize()
        return g2d

    for accumulate in (False, True):
        base = hs.into(start[accumulate])
        whole = {k: b.clone() for k, b in base.items()}
        whole2d = launch(whole, CANARY, accumulate)
        assert all(torch.isfinite(g).all() for g in whole2d) and all(torch.isfinite(b).all() for b in whole.values())
        union = {k: b.clone() for k, b in base.items()}
        for first, count in ranges:
            one = {k: b.clone() for k, b in base.items()}
            one2d = launch(one, CANARY, accumulate, first, count)
            inside = torch.zeros(P, dtype=torch.bool, device=gpu_device)
            inside[first:first + count] = True
            for k in one:
                assert torch.equal(one[k][inside], whole[k][inside]), (accumulate, first, k)
                assert torch.equal(one[k][~inside], base[k][~inside]), (accumulate, first, k, "written outside the range")
            for v in range(V):
                assert torch.equal(one2d[v][inside], whole2d[v][inside]), (accumulate, first, v)
                assert torch.all(one2d[v][~inside] == CANARY), (accumulate, first, v, "dL_dmeans2D written outside the range")
            launch(union, CANARY, accumulate, first, count)
        for k in union:
            assert torch.equal(union[k], whole[k]), (accumulate, k)


@pytest.mark.parametrize("D", [0, 2])
def test_batch_level_major_planes(D, gpu_device):
    """tgs_backward_batch_range_planes: dL_dsh level-major with a plane stride larger than 3 P (padding between the planes).  The planes hold
    the row-major result bit for bit, the padding stays bit for bit what it was, and at D = 0 only plane 0 is non-zero -- whole launch and ranges."""
    from diff_gaussian_rasterization import _C
    P, V, M = 1800, 9, 16
    cloud, cams, dLs = make_scene(P, V, D, M, False, 33, 2.0, False)
    hs = HipScene(cloud, cams, dLs, M, False, gpu_device)
    views = [hs.rendered(v) for v in range(V)]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    stride = (3 * P + 3) // 4 * 4 + 64
    rowmajor = hs.into(lambda s: torch.full(s, CANARY, device=gpu_device))
    hs.batch(views, rowmajor, accumulate=False)
    want = rowmajor["sh"]
    for ranges in ([(0, P)], [(0, 512), (512, 1024), (1536, P - 1536)]):
        planes = torch.full((M * stride,), CANARY, device=gpu_device)
        bufs = hs.into(lambda s: torch.full(s, CANARY, device=gpu_device))
        for first, count in ranges:
            arr, _g2d = _view_array(views, P, gpu_device, CANARY)
            _C.backward_batch_raw(stream, P, D, M, arr, V, hs.means.data_ptr(), hs.shs.data_ptr(), hs.scales.data_ptr(), 1.0, hs.rots.data_ptr(),
                                  bufs["opacities"].data_ptr(), bufs["means3D"].data_ptr(), planes.data_ptr(), bufs["scales"].data_ptr(),
                                  bufs["rotations"].data_ptr(), False, first=first, count=count, dsh_plane_stride=stride)
        torch.cuda.synchronize()
        pl = planes.view(M, stride)
        assert torch.all(pl[:, 3 * P:] == CANARY), "padding between the planes was written"
        for k in range(M):
            assert torch.equal(pl[k, :3 * P].view(P, 3), want[:, k, :]), k
        for k in ("means3D", "opacities", "scales", "rotations"):
            assert torch.equal(bufs[k], rowmajor[k]), k
        if D == 0:
            assert torch.all(pl[1:, :3 * P] == 0) and torch.any(pl[0, :3 * P] != 0)


def _leaves(cloud, dev, names):
    return {n: _t(cloud[n], dev).requires_grad_(True) for n in names}


def _settings(cam, D, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                         bg=_t(cam.bg, dev), scale_modifier=1.0, viewmatrix=_t(cam.viewmatrix, dev), projmatrix=_t(cam.projmatrix, dev),
                                         sh_degree=D, campos=_t(cam.campos, dev), prefiltered=False, debug=False)


def _check_against_oracle(images, grads, f64_views, f64, rep):
    for v, img in enumerate(images):
        e = util.rel_l2(img.detach().cpu().numpy(), f64_views[v]["color"])
        rep["color"] = max(rep.get("color", 0.0), e)
        assert e <= REL_TOL, f"view {v}: image rel-L2 to the double oracle {e:.3e}"
    for k, g in grads.items():
        e = rep[k] = util.rel_l2(g.detach().cpu().numpy().reshape(f64[k].shape), f64[k])
        assert e <= REL_TOL, f"{k}: rel-L2 to the double oracle {e:.3e} > {REL_TOL:.0e}"


# (D, forward group, cloud seed, recorded eta): SH stored at M = 16, rendered below degree 3
RUN_VIEWS_CASES = [(0, 1, 13, 4.1e-6), (0, 4, 13, 4.1e-6), (1, 1, 13, 4.1e-6), (1, 4, 13, 4.1e-6)]


@pytest.mark.parametrize("D,group,seed,eta_rec", RUN_VIEWS_CASES)
def test_run_views_below_the_stored_degree_vs_oracle(D, group, seed, eta_rec, gpu_device):
    """SyncFreeBatch.run_views -- the trainers' whole-batch path -- with SH stored for degree 3 and the step rendered at degree D
    (settings.sh_degree), the per-Gaussian forward one view per launch (group 1) and four (group 4: the all-views kernel, which the suite
    otherwise only runs at degree 3): every image and the summed parameter gradients against the double oracle; the coefficients above the
    active degree stay exactly 0 in .grad."""
    from diff_gaussian_rasterization import _C
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
    P, V = 3000, 5
    cloud, cams, dLs = make_scene(P, V, D, 16, False, seed, 2.0, False)
    eta, f64_views, f64 = scene_eta(cloud, cams, dLs, 16, False)
    assert eta <= 1.5 * eta_rec and 2.0 * eta <= REL_TOL, eta
    names = ("means3D", "opacities", "scales", "rotations", "shs")
    L = _leaves(cloud, gpu_device, names)
    flat = FlatGradients([L[n] for n in names])
    settings = [_settings(c, D, gpu_device) for c in cams]
    up = torch.stack([_t(d, gpu_device) for d in dLs])
    _C.set_forward_group(group)
    try:
        batch = SyncFreeBatch(granule=256, streams=2)
        for _ in range(3):                              # first batch synchronous (learns the bound), then the whole-batch path twice
            flat.flat.fill_(float("nan"))
            imgs = batch.run_views(settings, L["means3D"], L["opacities"], L["shs"], L["scales"], L["rotations"], lambda images: up, accumulate=False)
        assert batch.rejected == 0 and batch.capacity() is not None
    finally:
        _C.set_forward_group(2)                         # the default
    assert torch.all(L["shs"].grad[:, (D + 1) ** 2:] == 0), "dead SH coefficients must stay exactly 0"
    rep = {"eta": eta}
    grads = {"dL_dmeans3D": L["means3D"].grad, "dL_dopacity": L["opacities"].grad, "dL_dsh": L["shs"].grad, "dL_dscales": L["scales"].grad,
             "dL_drotations": L["rotations"].grad}
    _check_against_oracle([imgs[v] for v in range(V)], grads, f64_views, f64, rep)
    for v in range(V):
        e = util.rel_l2(batch.viewspace_grads[v].cpu().numpy(), f64_views[v]["dL_dmeans2D"])
        rep["dL_dmeans2D"] = max(rep.get("dL_dmeans2D", 0.0), e)
        assert e <= REL_TOL, (v, e)
    util.record_parity(f"batch_backward/run_views-D{D}-group{group}", rep)


@pytest.mark.parametrize("D,seed,eta_rec", [(2, 51, 4.0e-6), (0, 51, 3.9e-6)])
def test_run_with_cov3d_precomp_vs_oracle(D, seed, eta_rec, gpu_device):
    """SyncFreeBatch.run with a rasterize callback that passes cov3D_precomp: DeferredBackward.finish hands it to
    rasterize_gaussians_backward_batch, so the per-Gaussian half of the batch is k_preprocess_bwd_batch_split<false>.  The gradients on
    means3D, opacities, shs and cov3D_precomp against the sums of the double oracle."""
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch, rasterize_accumulate
    P, V = 2500, 4
    cloud, cams, dLs = make_scene(P, V, D, 16, False, seed, 2.0, True)
    eta, f64_views, f64 = scene_eta(cloud, cams, dLs, 16, True)
    assert eta <= 1.5 * eta_rec and 2.0 * eta <= REL_TOL, eta
    names = ("means3D", "opacities", "shs", "cov3D_precomp")
    L = _leaves(cloud, gpu_device, names)
    flat = FlatGradients([L[n] for n in names])
    settings = [_settings(c, D, gpu_device) for c in cams]
    up = [_t(d, gpu_device) for d in dLs]

    def rasterize(v, cap):
        return rasterize_accumulate(settings[v], means3D=L["means3D"], means2D=torch.zeros(P, 3, device=gpu_device, requires_grad=True),
                                    opacities=L["opacities"], shs=L["shs"], cov3D_precomp=L["cov3D_precomp"], r_capacity=cap, return_meta=True)

    batch = SyncFreeBatch(granule=256, streams=2)
    flat.zero_()
    batch.run(range(V), rasterize, lambda v, img: up[v])        # synchronous: learns the bound
    assert batch.capacity() is not None
    flat.zero_()
    imgs = batch.run(range(V), rasterize, lambda v, img: up[v])  # deferred: one batch pass for the four views
    assert batch.rejected == 0
    assert torch.all(L["shs"].grad[:, (D + 1) ** 2:] == 0)
    rep = {"eta": eta}
    grads = {"dL_dmeans3D": L["means3D"].grad, "dL_dopacity": L["opacities"].grad, "dL_dsh": L["shs"].grad, "dL_dcov3D": L["cov3D_precomp"].grad}
    _check_against_oracle(imgs, grads, f64_views, f64, rep)
    util.record_parity(f"batch_backward/run_cov3d-D{D}", rep)
