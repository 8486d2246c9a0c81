"""The loss kernels (csrc/tgs_loss.hip) pixel by pixel: every seam of the streaming SSIM kernels, smooth images, per-image batches, non-finite
input, and the pointwise kernel element by element.  tests/test_loss.py and tests/test_loss_ext.py look at the scalar value and at the rel-L2
of the whole gradient; one wrong pixel, one wrong seam column or a partial sum credited to the neighbouring image passes those.

THE JUDGE (oracle/loss_ref.py: judge, pixel_bars).  want = float64 autograd of oracle/loss_ref.py, ref32 = the same in fp32 on the CPU,
got = the kernel.  Per pixel
    |got - want|(p) <= max(M * env(p), 2^-20 * max|want|),   env = max |ref32 - want| over the 21 x 21 pixels around p,   M = 4
-- the reference's own fp32 noise where the pixel's 11 x 11 window and its adjoint reach, with a floor for pixels whose true gradient is ~0
and where ref32 happens to be exact -- and per tensor: value and gradient rel-L2 within max(1e-5, 2 eta) of want, eta = the distance of ref32 from want in the same measure.
M and the floor are measured against the reference, not the kernel: test_fp32_restatement_is_within_the_pixel_bars runs an fp32 numpy
restatement of the kernels' FORMULATION (loss_ref.kernel_formulation_fp32: four maps, separable, (SS - mu1^2 - mu2^2) + C2; exact division,
no FMA) through the same judge on every case below except the 1080p one, no pixel left out; what M = 4 leaves above that covers FMA contraction
and v_rcp_f32 (1 ulp on 1 / D1, 1 / D2).  test_judge_rejects_what_the_whole_tensor_bar_accepts plants the errors the old bar cannot see.

THE CASES.  Seams: WIDTHS x HEIGHTS as one plane of white noise (test_loss_ext._inputs: there the bar is tightest), dssim_factor 1.0 through
loss.ssim and 0.2 through l1_ssim_loss and l1_ssim_value_and_grad; test_seam_table_covers_the_kernels_seams derives what the table has to
contain from the kernels' constants.  (Height 7 is added to the table the issue gives: it is the one length of a last group of rows, 6, that
the others leave out.)  PLANES: some of them again as [C,H,W] and as [B,C,H,W] with 2, 7 and 900 planes.  PER_IMAGE: batches of unlike images
(noise sigma 0.01 ... 0.3) with unlike upstream weights.  REGIMES at 3 x 130 x 230 (smooth also at 3 x 1080 x 1920 and as a per-image batch):
    smooth     low-frequency sinusoids saturated at 0 and 1, constant patches, a band of rows with pred == gt, pred - gt ~ 1e-2 smooth + 2e-3 noise
    steps      piecewise constant (a patchwork of levels) with step edges, pred = gt + 1e-3 on half of it, misregistered by a pixel on the rest
    zero, same all zero; pred == gt everywhere on white noise (map == 1, gradient == 0; identical_image says why not on the smooth image)
    range      white noise x 3 - 0.5: unclamped renderer output
eta (the reference's own fp32 rel-L2 from float64; dssim_factor 0.2 / 1.0) as the CPU run of this module prints it, and next to it the rel-L2 of the
restatement of the kernels' formulation: white noise (the seam table, at most) 4.3e-7 / 1.9e-6, restatement 1.7e-7 / 1.8e-6; smooth 3.8e-5 / 4.6e-5,
restatement 1.9e-5 / 2.4e-5; steps 1.2e-4 / 1.6e-4, restatement 3.8e-5 / 4.9e-5; range 1.1e-7 / 1.2e-6, restatement 5.8e-8 / 5.2e-7; the smooth
per-image batch 3.4e-5 / 4.0e-5, restatement 1.8e-5 / 2.1e-5.  The restatement's worst pixel: 0.90 x its bar over the seam table (133 x 1; 0.53 at
most for widths above 2), 0.42 x over the regimes.  The GPU run records the kernels' figures with util.record_parity (loss_pixelwise_*); none are quoted here yet: the GPU half of this
module has not run on an MI355X at the time of writing.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import loss_ref
from tests import util
from tests.test_loss_ext import _inputs

# the streaming kernels' geometry as csrc/tgs_loss.hip states it
OUT_COLS, HALO, SEG_ROWS, GROUP, STRIPS_PER_WG = 54, 5, 64, 11, 4
WIDTHS = (1, 2, 5, 6, 10, 11, 12, 49, 53, 54, 55, 59, 60, 107, 108, 109, 215, 216, 217, 221, 271)
HEIGHTS = (1, 2, 5, 6, 7, 10, 11, 12, 58, 59, 63, 64, 65, 69, 70, 74, 75, 128, 129, 133)
FACTORS = (0.2, 1.0)
PLANES = ((3, 65, 55), (3, 129, 217), (3, 5, 6), (3, 12, 271), (2, 1, 64, 54), (1, 7, 70, 109), (7, 1, 6, 221), (300, 3, 11, 60), (100, 9, 65, 55))
PER_IMAGE = ((2, 3, 130, 230), (5, 1, 70, 271), (5, 3, 70, 271), (2, 1, 130, 230))
REGIME_SHAPE = (3, 130, 230)
VALUE_RTOL = 1e-5


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def unlike_images(shape, seed=None):
    """a batch whose images differ in the first digit of their SSIM: per-image noise sigma from 0.01 to 0.3"""
    rng = np.random.default_rng(sum(shape) + 1 if seed is None else seed)
    gt = rng.uniform(0, 1, shape).astype(np.float32)
    sigma = np.geomspace(0.01, 0.3, shape[0]).reshape(-1, 1, 1, 1)
    return np.clip(gt + sigma * rng.normal(0, 1, shape), 0, 1).astype(np.float32), gt


def unlike_weights(B):
    return np.array([0.375, 1.75, 0.8125, 2.5, 1.125][:B])


def smooth_pair(shape, seed=11):
    rng = np.random.default_rng(seed)
    C, H, W = shape[-3:]
    lead = shape[:-3]
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, lead + (C, 1, 1))
    gt = 0.5 + 0.7 * np.sin(2 * np.pi * 1.5 * x + ph) * np.cos(2 * np.pi * 1.1 * y + 0.5 * ph)        # leaves [0, 1]: saturates below
    gt = np.clip(gt, 0, 1)
    gt[..., H // 8:H // 8 + max(H // 6, 1), W // 10:W // 10 + max(W // 5, 1)] = 0.25                 # constant patches
    gt[..., H // 2:H // 2 + max(H // 8, 1), W // 2:W // 2 + max(W // 7, 1)] = 0.75
    delta = 1e-2 * np.sin(2 * np.pi * 0.8 * x + 1.0) * np.cos(2 * np.pi * 0.6 * y) + 2e-3 * rng.normal(0, 1, gt.shape)
    pred = np.clip(gt + delta, 0, 1)
    band = slice((5 * H) // 8, (5 * H) // 8 + max(H // 10, 1))
    pred[..., band, :] = gt[..., band, :]                                                              # a band of rows with pred == gt exactly
    gt, pred = gt.astype(np.float32), pred.astype(np.float32)
    pred[..., band, :] = gt[..., band, :]
    return pred, gt


def steps_pair(shape, seed=5, patch=16):
    """A patchwork of constant levels (step edges every `patch` pixels, blocks saturated at 0 and 1); pred = gt + 1e-3 on the left half and the
    same patchwork one pixel off on the right half.  No part has pred == gt: there the reference's five windows cancel identically
    (sigma1^2 + sigma2^2 == 2 sigma12, gradient exactly 0, envelope 0) while x^2 + y^2 in ONE window leaves ~ulp(x^2) / C2 of the map, and
    on an image whose gradient is small everywhere (pred - gt = 1e-3) that is 2 ... 5 x the floor for the RESTATEMENT already (measured with the
    middle third left untouched) -- a property of the four-map formulation on such an image, not something the kernel could be held to here.
    pred == gt on flat patches is judged where the image has gradients of ordinary size: the smooth regime's patches and band."""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    levels = rng.uniform(0, 1, (C, -(-H // patch) + 1, -(-W // patch) + 1)).astype(np.float32)
    full = np.kron(levels, np.ones((patch, patch), np.float32))
    gt = full[:, :H, :W].copy()
    gt[1, H // 4:H // 4 + 20, W // 2:W // 2 + 31] = 0.0
    gt[2, H // 2:H // 2 + 25, W // 8:W // 8 + 40] = 1.0
    pred = gt.copy()
    pred[:, :, :W // 2] += np.float32(1e-3)
    pred[:, :, W // 2:] = full[:, 1:H + 1, 1:W + 1][:, :, W // 2:]
    return pred, gt


def range_pair(shape):
    pred, gt = _inputs(shape, seed=77)
    return (pred * 3 - 0.5).astype(np.float32), (gt * 3 - 0.5).astype(np.float32)


def _poke_nan(pair, index):
    pred, gt = pair
    pred = pred.copy()
    pred[index] = np.nan
    return pred, gt


NAN_SHAPE = (2, 75, 120)
NAN_PIXELS = {"corner": (0, 0, 0), "edge": (1, 30, 119), "seam": (0, 64, 54)}         # row 64: first of the second segment; column 54: first of the second strip


class Case:
    def __init__(self, name, make, per_image=False, weights=None):
        self.name, self.make, self.per_image, self.weights = name, make, per_image, weights

    def __repr__(self):
        return self.name


def seam_cases(width):
    return [Case(f"seam_{h}x{width}", functools.partial(_inputs, (1, h, width))) for h in HEIGHTS]


def planes_cases():
    return [Case("planes_" + "x".join(map(str, s)), functools.partial(_inputs, s)) for s in PLANES]


def per_image_cases():
    cs = [Case("per_image_" + "x".join(map(str, s)), functools.partial(unlike_images, s), True, unlike_weights(s[0])) for s in PER_IMAGE]
    return cs + [Case("per_image_smooth_2x3x130x230", functools.partial(smooth_pair, (2,) + REGIME_SHAPE), True, unlike_weights(2))]


def regime_cases():
    return [Case("regime_smooth", functools.partial(smooth_pair, REGIME_SHAPE)), Case("regime_steps", functools.partial(steps_pair, REGIME_SHAPE)),
            Case("regime_range", functools.partial(range_pair, REGIME_SHAPE))]


def nan_free_case():
    return Case("nan_free_" + "x".join(map(str, NAN_SHAPE)), functools.partial(_inputs, NAN_SHAPE, 21))


GROUPS = {**{f"seams_w{w}": functools.partial(seam_cases, w) for w in WIDTHS}, "planes": planes_cases, "per_image": per_image_cases, "regimes": regime_cases,
          "nan_free": lambda: [nan_free_case()]}
SMOOTH_1080P = Case("regime_smooth_3x1080x1920", functools.partial(smooth_pair, (3, 1080, 1920)))


# ------------------------------------------------------------------------------------------------------------------------------------
# a case through the judge.  A producer returns [(label, out, grad, weight)]: `out` the [3] or [B,3] values (loss, ssim, l1; NaN = this entry
# point does not return it), `grad` the gradient of sum_b weight_b * loss_b (weight a scalar or one per image), in numpy.
# ------------------------------------------------------------------------------------------------------------------------------------
def _per_image_scale(weight, shape):
    w = np.asarray(weight, np.float64)
    return w.reshape((-1,) + (1,) * (len(shape) - 1)) if w.ndim else w


def run_case(case, f, producer, record=None):
    """-> the worst report of the case's results.  The reference's gradient is linear in the upstream weight, so want and ref32 are evaluated
    once with weight 1 and scaled in float64."""
    pred, gt = case.make()
    out_w, grad_w = loss_ref.reference_value_and_grad(pred, gt, f, torch.float64, per_image=case.per_image)
    out_32, grad_32 = loss_ref.reference_value_and_grad(pred, gt, f, torch.float32, per_image=case.per_image)
    value_bar = np.maximum(VALUE_RTOL, 2.0 * np.abs(out_32 - out_w) / np.abs(out_w))       # the rule of the gradient's rel-L2, per value
    worst = None
    for label, out, grad, weight in producer(case, pred, gt, f):
        s = _per_image_scale(weight, grad_w.shape)
        rep = loss_ref.judge(grad, grad_w * s, grad_32 * s)
        out = np.asarray(out, np.float64)
        have = ~np.isnan(out)
        if f == 1.0:
            have[..., 0] = False                                 # the value at dssim_factor 1 is the SSIM: loss = 1 - ssim cancels (1 ulp of the SSIM of a 2-pixel image is 1e-5 of it)
        value_rel = float(np.max(np.abs(out[have] - out_w[have]) / np.abs(out_w[have]))) if have.any() else 0.0
        value_ok = np.all(np.abs(out[have] - out_w[have]) <= value_bar[have] * np.abs(out_w[have]))
        rep["value_rel"] = value_rel
        print(f"{case.name} f={f} {label}: worst pixel {rep['worst']:.3g} x bar at {rep['where']}, {rep['over']} of {rep['pixels']} over; "
              f"rel-L2 {rep['rel_l2']:.3g} (eta {rep['eta']:.3g}, bar {rep['rel_l2_bar']:.3g}); value rel {value_rel:.3g}")
        assert rep["over"] == 0 and rep["worst"] <= 1.0, (case.name, f, label, rep)
        assert rep["rel_l2"] <= rep["rel_l2_bar"], (case.name, f, label, rep)
        assert value_ok, (case.name, f, label, out, out_w, value_bar)
        if worst is None or rep["worst"] > worst["worst"]:
            worst = dict(rep, label=label)
    if record:
        util.record_parity(f"{record}_{case.name}_f{f}", {k: worst[k] for k in ("worst", "rel_l2", "eta", "value_rel")}, {"label": worst["label"], "where": worst["where"]})
    return worst


def restatement(case, pred, gt, f):
    out, grad = loss_ref.kernel_formulation_fp32(pred, gt, f, per_image=case.per_image)
    res = [("restatement", out, grad, 1.0)]
    if case.weights is not None:
        out, grad = loss_ref.kernel_formulation_fp32(pred, gt, f, upstream=case.weights, per_image=True)
        res.append(("restatement, weights", out, grad, case.weights))
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the bars without the code under test
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_fp32_restatement_is_within_the_pixel_bars(group):
    """every case of the tables (the 1080p one is left to the GPU run), both factors, no pixel left out"""
    worst = [run_case(case, f, restatement) for case in GROUPS[group]() for f in FACTORS]
    print(f"{group}: worst pixel {max(r['worst'] for r in worst):.3g} x bar, eta <= {max(r['eta'] for r in worst):.3g}")


def test_seam_table_covers_the_kernels_seams():
    """from the kernels' constants: a wave owns OUT_COLS output columns (+ HALO on either side), STRIPS_PER_WG waves make a workgroup, a wave
    walks SEG_ROWS output rows in groups of GROUP input rows"""
    assert OUT_COLS + 2 * HALO == 64 and GROUP == 2 * HALO + 1
    nstrips = {w: -(-w // OUT_COLS) for w in WIDTHS}
    live = {w - OUT_COLS * (nstrips[w] - 1) for w in WIDTHS}                    # output columns of the last strip
    assert live >= {1, HALO, HALO + 1, OUT_COLS - 1, OUT_COLS}, live
    assert {n % STRIPS_PER_WG for n in nstrips.values()} == {0, 1, 2, 3}      # waves past the last strip: 0, 3, 2, 1 of them write zero partials
    assert {-(-n // STRIPS_PER_WG) for n in nstrips.values()} >= {1, 2}       # one and several workgroups along x
    assert STRIPS_PER_WG * OUT_COLS in WIDTHS and STRIPS_PER_WG * OUT_COLS + 1 in WIDTHS
    last_rows = {h - SEG_ROWS * (-(-h // SEG_ROWS) - 1) for h in HEIGHTS}       # output rows of the last segment
    assert last_rows >= {1, HALO, HALO + 1, SEG_ROWS - 1, SEG_ROWS}, last_rows
    assert {-(-h // SEG_ROWS) for h in HEIGHTS} == {1, 2, 3}
    # a segment of n output rows reads n + 2 HALO input rows in whole groups of GROUP: the last group holds 1 ... GROUP live rows (the rest is
    # evaluated and never stored), each of which is another instantiation stats_row<P> / grad_row<P> finishing the segment's last output row
    seg_rows = last_rows | ({SEG_ROWS} if max(HEIGHTS) > SEG_ROWS else set())
    assert {(n + 2 * HALO - 1) % GROUP + 1 for n in seg_rows} == set(range(1, GROUP + 1))
    assert {w for w in WIDTHS if w < GROUP} >= {1, 2, HALO, HALO + 1, 2 * HALO} and {h for h in HEIGHTS if h < GROUP} >= {1, 2, HALO, HALO + 1, 2 * HALO}
    # a last segment that lies wholly inside the previous segment's halo
    assert {h % SEG_ROWS for h in HEIGHTS if h > SEG_ROWS} >= {1, HALO}
    for shape in PLANES:
        assert int(np.prod(shape[:-2])) in (2, 3, 7, 900)
    assert {int(np.prod(s[:-2])) for s in PLANES} == {2, 3, 7, 900}
    for (B, C, H, W) in PER_IMAGE:
        assert -(-W // OUT_COLS) % STRIPS_PER_WG != 0 and -(-W // OUT_COLS) > STRIPS_PER_WG
    assert {s[0] for s in PER_IMAGE} == {2, 5} and {s[1] for s in PER_IMAGE} == {1, 3}
    for index in NAN_PIXELS.values():
        assert all(i < n for i, n in zip(index, NAN_SHAPE))
    assert NAN_PIXELS["seam"][1:] == (SEG_ROWS, OUT_COLS)


def test_unlike_images_are_unlike():
    """per image: SSIMs that differ in the first digit and weights that all differ, so that a partial credited to the wrong image or a gradient
    scaled by the neighbour's weight moves a value by far more than its bar"""
    for shape in PER_IMAGE:
        pred, gt = unlike_images(shape)
        out, grad = loss_ref.reference_value_and_grad(pred, gt, 1.0, per_image=True)
        s = np.sort(out[:, 1])
        assert np.all(np.diff(s) > 100 * VALUE_RTOL) and s[-1] - s[0] > 0.2, s
        w = unlike_weights(shape[0])
        assert len(set(w.tolist())) == shape[0] and np.all(np.abs(np.diff(np.sort(w))) > 0.1)
        # the neighbour's weight on image 0 is outside image 0's bars
        _o, g32 = loss_ref.reference_value_and_grad(pred, gt, 1.0, torch.float32, per_image=True)
        swapped = grad * _per_image_scale(np.roll(w, 1), grad.shape)
        rep = loss_ref.judge(swapped, grad * _per_image_scale(w, grad.shape), g32 * _per_image_scale(w, grad.shape))
        assert rep["worst"] > 1e3


def test_judge_rejects_what_the_whole_tensor_bar_accepts():
    """(a) one pixel 1 % off, (b) seam column 54 of one plane 0.05 % off, (c) output row 64 shifted by one column, planted into the float64
    gradient of a 3 x 1080 x 1920 noise case: the judge rejects each; rel-L2 <= 1e-5, the bar of tests/test_loss*.py, accepts (a) and (b)."""
    pred, gt = _inputs((3, 1080, 1920))
    _o, want = loss_ref.reference_value_and_grad(pred, gt, 0.2, torch.float64)
    _o, ref32 = loss_ref.reference_value_and_grad(pred, gt, 0.2, torch.float32)
    bars = loss_ref.pixel_bars(want, ref32)
    clean = loss_ref.judge(ref32, want, ref32, bars=bars)
    assert clean["over"] == 0 and loss_ref.passes(clean)          # (the reference's own fp32 gradient is inside its envelope by construction)
    typical = np.median(np.abs(want))
    row = np.abs(np.abs(want[1, 500]) - typical)
    one = want.copy(); one[1, 500, int(row.argmin())] *= 1.01
    col = want.copy(); col[2, :, OUT_COLS] *= 1.0005
    shift = want.copy(); shift[0, SEG_ROWS, 1:] = want[0, SEG_ROWS, :-1]
    for label, planted, hidden in (("one pixel", one, True), ("seam column", col, True), ("shifted row", shift, False)):
        d = util.rel_l2(planted, want)
        rep = loss_ref.judge(planted, want, ref32, bars=bars)
        print(f"{label}: rel-L2 {d:.3g}, judge: {rep['over']} pixels over, worst {rep['worst']:.3g} x bar")
        assert (d <= 1e-5) == hidden, (label, d)                  # the shifted row is 4e-2 in rel-L2: seen by the old bar on the gradient, not on the value
        assert rep["over"] >= 1 and rep["worst"] > 10.0 and not loss_ref.passes(rep), (label, rep)
    assert (loss_ref.judge(one, want, ref32, bars=bars)["over"], loss_ref.judge(col, want, ref32, bars=bars)["over"]) == (1, 1080)


def test_reference_spreads_a_nan_over_its_reach_only():
    """what the GPU test compares against: in float64 a NaN in pred makes the 21 x 21 pixels around it non-finite (its own plane only) and
    leaves every other pixel what it is without the NaN; the restatement's non-finite set is inside that"""
    clean = nan_free_case().make()
    _o, want_clean = loss_ref.reference_value_and_grad(*clean, 0.2)
    for name, index in NAN_PIXELS.items():
        pred, gt = _poke_nan(clean, index)
        _o, want = loss_ref.reference_value_and_grad(pred, gt, 0.2)
        box = np.zeros(NAN_SHAPE, bool)
        c, y, x = index
        box[c, max(y - 10, 0):y + 11, max(x - 10, 0):x + 11] = True
        assert np.array_equal(~np.isfinite(want), box), name
        np.testing.assert_allclose(want[~box], want_clean[~box], rtol=1e-12, atol=0)
        _o, got = loss_ref.kernel_formulation_fp32(pred, gt, 0.2)
        assert not np.any(~np.isfinite(got) & ~box), name


def identical_image(what):
    """regime (c): all zero; pred == gt everywhere -- a white-noise image.  Not the smooth image: on its patches saturated at 1 the four-map
    formulation leaves a gradient of up to 6.8 x the smooth regime's floor (1.1e-9 at 3 x 130 x 230; the restatement, so the formulation and not
    the kernel) where the reference's five windows cancel to exactly 0 -- x^2 + y^2 in one window rounds at ulp(2) against C2 = 9e-4.  The
    steps image against itself: 10 x.  White noise: 0.05 x."""
    return np.zeros(REGIME_SHAPE, np.float32) if what == "zero" else _inputs(REGIME_SHAPE)[1]


def smooth_floor():
    return {f: loss_ref.PIXEL_FLOOR * np.abs(loss_ref.reference_value_and_grad(*smooth_pair(REGIME_SHAPE), f)[1]).max() for f in FACTORS}


@pytest.mark.parametrize("what", ["zero", "same"])
def test_fp32_restatement_on_identical_images(what):
    a = identical_image(what)
    floor = smooth_floor()
    for f in FACTORS:
        out3, grad = loss_ref.kernel_formulation_fp32(a, a.copy(), f)
        print(f"{what} f={f}: out3 {out3}, max |gradient| {np.abs(grad).max():.3g} (floor {floor[f]:.3g})")
        assert abs(out3[1] - 1.0) <= 1e-6 and out3[2] == 0.0 and abs(out3[0]) <= 1e-6
        assert np.abs(grad).max() <= floor[f]


def pixel_want(kind, x, y, weight):
    """float64 gradient of sum_b weight_b * mean_b over the last axis of |x - y| or (x - y)^2, from the fp32 inputs"""
    d = x.astype(np.float64) - y.astype(np.float64)
    n = x.shape[-1]
    w = np.asarray(weight, np.float64).reshape(-1, 1) if np.ndim(weight) else float(weight)
    return (np.sign(d) if kind == "l1" else 2.0 * d) * (w / n)


def assert_every_element(got, want, kind, label):
    """s * sign(d) or s * d with s = fp32(fp32 scale * upstream) and d = x - y: every element within 4 * 2^-24 of float64 (L1: exactly 0 at x == y)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, label
    bad = np.abs(got - want) > 4.0 * 2.0 ** -24 * np.abs(want)
    if bad.any():
        i = np.unravel_index(int(bad.argmax()), bad.shape)
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} elements off, first at {i}: got {got[i]!r}, want {want[i]!r}")
    if kind == "l1":
        assert np.all(got[want == 0.0] == 0.0), label


def test_element_bar_holds_for_fp32_arithmetic():
    """the pointwise bar from the number format: the kernel's three products and one difference, each rounded to fp32, stay inside it"""
    rng = np.random.default_rng(3)
    x, y = rng.uniform(0, 1, (7, 7021)).astype(np.float32), rng.uniform(0, 1, (7, 7021)).astype(np.float32)
    x[:, ::5] = y[:, ::5]
    w = rng.uniform(0.25, 2.0, 7).astype(np.float32)
    s2, s1 = (np.float32(2.0 / 7021) * w).reshape(-1, 1), (np.float32(1.0 / 7021) * w).reshape(-1, 1)
    d = x - y
    assert_every_element(s2 * d, pixel_want("l2", x, y, w), "l2", "fp32 l2")
    assert_every_element(s1 * np.sign(d), pixel_want("l1", x, y, w), "l1", "fp32 l1")
    with pytest.raises(AssertionError):
        assert_every_element(s2 * d * np.float32(1 + 2 ** -21), pixel_want("l2", x, y, w), "l2", "off by 8 ulp")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _cuda(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _nan3(B=None, **known):
    out = np.full((3,) if B is None else (B, 3), np.nan)
    for i, v in known.items():
        out[..., "loss ssim l1".split().index(i)] = v
    return out


def _images_backward(p, g, f, upstream, per_image):
    """tgs_l1_ssim_images (the statistics pass fills the workspace) + tgs_l1_ssim_images_backward: the argument combinations without a Python form"""
    from youreditableavatar_amd.loss import _lib
    B, Cn, H, W = p.shape
    nbytes = int(_lib.tgs_l1_ssim_images_workspace_bytes(B, Cn, H, W))
    ws, out, grad = torch.empty(nbytes, dtype=torch.uint8).cuda(), torch.empty(B, 3).cuda(), torch.full_like(p, float("nan"))
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.tgs_l1_ssim_images(st, B, Cn, H, W, p.data_ptr(), g.data_ptr(), f, out.data_ptr(), None, ws.data_ptr(), nbytes) == 0
    assert _lib.tgs_l1_ssim_images_backward(st, B, Cn, H, W, p.data_ptr(), g.data_ptr(), f, upstream.data_ptr() if upstream is not None else None, per_image,
                                            grad.data_ptr(), ws.data_ptr(), nbytes) == 0
    return out.cpu().numpy(), grad.cpu().numpy()


def kernels(case, pred, gt, f):
    """the case through every public entry point that takes this dssim_factor"""
    from youreditableavatar_amd import loss
    g = _cuda(gt)
    res = []
    if not case.per_image:
        if f == 1.0:
            p = _cuda(pred).requires_grad_(True)
            v = loss.ssim(p, g)
            (0.5 * v).backward()                                # d ssim = - d loss at dssim_factor 1; 0.5 scales exactly
            res.append(("ssim", _nan3(ssim=v.item()), -p.grad.cpu().numpy(), 0.5))
        else:
            p = _cuda(pred).requires_grad_(True)
            v = loss.l1_ssim_loss(p, g, f)
            (0.5 * v).backward()
            res.append(("l1_ssim_loss", _nan3(loss=v.item()), p.grad.cpu().numpy(), 0.5))
        out3, grad = loss.l1_ssim_value_and_grad(_cuda(pred), g, f)
        res.append(("l1_ssim_value_and_grad", out3.cpu().numpy(), grad.cpu().numpy(), 1.0))
        return res
    B, w = pred.shape[0], case.weights
    if f == 1.0:
        p = _cuda(pred).requires_grad_(True)
        s = loss.ssim(p, g, size_average=False)
        (s * _cuda(w)).sum().backward()
        res.append(("ssim per image", _nan3(B, ssim=s.detach().cpu().numpy()), -p.grad.cpu().numpy(), w.astype(np.float32)))
    out, grad = loss.l1_ssim_value_and_grad(_cuda(pred), g, f, per_image=True)
    res.append(("l1_ssim_value_and_grad per image", out.cpu().numpy(), grad.cpu().numpy(), 1.0))
    for label, up, per, weight in (("images_backward, weights", _cuda(w), 1, w.astype(np.float32)), ("images_backward, scalar", _cuda([0.375]), 0, 0.375),
                                   ("images_backward, NULL", None, 0, 1.0)):
        o, gr = _images_backward(_cuda(pred), g, f, up, per)
        res.append((label, o, gr, weight))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_gpu_every_pixel_is_within_the_bars(group):
    worst, failed = {f: [] for f in FACTORS}, []
    for case in GROUPS[group]():
        for f in FACTORS:
            try:                                                # every case of the group is run and printed before the first failure is raised
                worst[f].append(run_case(case, f, kernels, record=None if group.startswith("seams") else "loss_pixelwise"))
            except AssertionError as e:
                failed.append(str(e)[:600])
    if group.startswith("seams"):                                # 840 cases: one line per width and factor, its extremes
        for f, rs in worst.items():
            if rs:
                top = max(rs, key=lambda r: r["worst"])
                util.record_parity(f"loss_pixelwise_{group}_f{f}", {"worst": top["worst"], "rel_l2": max(r["rel_l2"] for r in rs), "eta": max(r["eta"] for r in rs),
                                                                     "value_rel": max(r["value_rel"] for r in rs)}, {"cases": len(rs), "where": top["where"]})
    assert not failed, f"{len(failed)} of {len(GROUPS[group]()) * len(FACTORS)} cases: " + " | ".join(failed[:4])


@pytest.mark.gpu
def test_gpu_smooth_1080p_every_pixel():
    for f in FACTORS:
        run_case(SMOOTH_1080P, f, kernels, record="loss_pixelwise")


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["zero", "same"])
def test_gpu_identical_images_give_one_and_no_gradient(what):
    """map == 1, gradient == 0: the value is 1 to 1e-6 and every gradient element is below the floor of the smooth regime's bars"""
    from youreditableavatar_amd import loss
    floor = smooth_floor()
    p = _cuda(identical_image(what))
    for f in FACTORS:
        out3, grad = loss.l1_ssim_value_and_grad(p, p.clone(), f)
        out3, worst = out3.cpu().numpy(), float(grad.abs().max())
        print(f"{what} f={f}: out3 {out3}, max |gradient| {worst:.3g} (floor {floor[f]:.3g})")
        assert abs(out3[1] - 1.0) <= 1e-6 and out3[2] == 0.0 and abs(out3[0]) <= 1e-6
        assert torch.isfinite(grad).all() and worst <= floor[f]
        util.record_parity(f"loss_pixelwise_regime_{what}_f{f}", {"max_abs_gradient": worst, "floor": float(floor[f]), "ssim_minus_1": float(out3[1] - 1.0)})
    q = p.clone().requires_grad_(True)
    s = loss.ssim(q, p)
    s.backward()
    assert abs(s.item() - 1.0) <= 1e-6 and float(q.grad.abs().max()) <= floor[1.0]
    if what == "same":                                          # for the record, not asserted: the smooth image against itself (see identical_image)
        p = _cuda(smooth_pair(REGIME_SHAPE)[1])
        for f in FACTORS:
            _o, grad = loss.l1_ssim_value_and_grad(p, p.clone(), f)
            util.record_parity(f"loss_pixelwise_smooth_against_itself_f{f}", {"max_abs_gradient": float(grad.abs().max()), "floor": float(floor[f])})


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NAN_PIXELS))
def test_gpu_a_nan_stays_within_its_reach(name):
    """the kernels load every row from a clamped address and multiply by 0 or 1: NaN x 0 must not leave the reach the reference gives the NaN"""
    from youreditableavatar_amd import loss
    clean = nan_free_case().make()
    pred, gt = _poke_nan(clean, NAN_PIXELS[name])
    for f in FACTORS:
        _o, want_clean = loss_ref.reference_value_and_grad(*clean, f)
        _o, ref32_clean = loss_ref.reference_value_and_grad(*clean, f, torch.float32)
        _o, want = loss_ref.reference_value_and_grad(pred, gt, f)
        finite = np.isfinite(want)
        bars = loss_ref.pixel_bars(want_clean, ref32_clean)
        _out3, grad = loss.l1_ssim_value_and_grad(_cuda(pred), _cuda(gt), f)
        got = grad.cpu().numpy().astype(np.float64)
        stray = ~np.isfinite(got) & finite
        assert not stray.any(), (name, f, int(stray.sum()), np.argwhere(stray)[:5].tolist())
        ratio = np.abs(got - want_clean)[finite] / bars[finite]
        print(f"nan at {name} f={f}: {int((~np.isfinite(got)).sum())} non-finite gradient pixels (reference {int((~finite).sum())}), worst other pixel {ratio.max():.3g} x bar")
        assert ratio.max() <= 1.0, (name, f, float(ratio.max()))
        util.record_parity(f"loss_pixelwise_nan_{name}_f{f}", {"worst": float(ratio.max()), "nonfinite": int((~np.isfinite(got)).sum()), "nonfinite_reference": int((~finite).sum())})


# ---- the pointwise kernel, element by element ----
PX_STEP = 4 * 1024 * 2048                                       # elements one round of the float4 grid takes: 1024 float4 per workgroup x 2048 workgroups
ONE_IMAGE_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 4100, PX_STEP - 4, PX_STEP, PX_STEP + 4, PX_STEP + 7)
IMAGES = (2, 3, 1000, 2047, 2048, 2049, 5000, 65535)
IMAGE_N = (1, 5, 1028, 7021)
MAX_ELEMS = 80_000_000                                          # three fp32 tensors on the device under ~1 GB


def _pixel_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    gt = rng.random(shape, dtype=np.float32)
    pred = np.clip(gt + np.float32(0.1) * rng.standard_normal(shape, dtype=np.float32), 0, 1)
    pred.reshape(-1)[::7] = gt.reshape(-1)[::7]                 # x == y exactly on every seventh element
    return pred, gt


def _pixel_backward(kind, p, g, images, n, upstream, per_image, grad=None):
    from youreditableavatar_amd.loss import _lib
    grad = torch.full_like(p, float("nan")) if grad is None else grad
    assert _lib.tgs_pixel_loss_backward(torch.cuda.current_stream().cuda_stream, {"l1": 0, "l2": 1}[kind], images, n, p.data_ptr(), g.data_ptr(),
                                        upstream.data_ptr() if upstream is not None else None, per_image, grad.data_ptr()) == 0
    return grad


@pytest.mark.gpu
@pytest.mark.parametrize("n", ONE_IMAGE_N)
def test_gpu_pointwise_one_image_every_element(n):
    from youreditableavatar_amd import loss
    pred, gt = _pixel_inputs((1, n), seed=n)
    p, g = _cuda(pred[0]), _cuda(gt[0])
    q = p.clone().requires_grad_(True)
    v = loss.l2_loss(q, g)
    (3.0 * v).backward()                                        # the incoming gradient as a device scalar
    want_v = {"l2": ((pred.astype(np.float64) - gt) ** 2).mean(), "l1": np.abs(pred.astype(np.float64) - gt).mean()}
    np.testing.assert_allclose(v.item(), want_v["l2"], rtol=1e-5)
    assert_every_element(q.grad.cpu().numpy(), pixel_want("l2", pred, gt, 3.0)[0], "l2", f"l2_loss n={n}")
    for kind in ("l1", "l2"):
        val, grad = loss.pixel_value_and_grad(p, g, kind)
        np.testing.assert_allclose(val.item(), want_v[kind], rtol=1e-5)
        assert_every_element(grad.cpu().numpy(), pixel_want(kind, pred, gt, 1.0)[0], kind, f"pixel_value_and_grad {kind} n={n}")
        up = _cuda([1.375])
        assert_every_element(_pixel_backward(kind, p, g, 1, n, up, 0).cpu().numpy(), pixel_want(kind, pred, gt, 1.375)[0], kind, f"backward {kind} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("images", IMAGES)
def test_gpu_pointwise_per_image_every_element(images):
    """the grid's cap on workgroups per image truncates (2048 / 3, 2048 / 1000), is 1 (2047 images and more: one workgroup walks a whole image),
    and the 4-byte path (n % 4 != 0 with several images) runs with one and with many workgroups per image"""
    from youreditableavatar_amd import loss
    for n in IMAGE_N:
        if images * n > MAX_ELEMS:
            assert (images, n) == (65535, 7021)                 # 460 M elements: 1.8 GB per tensor
            continue
        pred, gt = _pixel_inputs((images, n), seed=images + n)
        p, g = _cuda(pred), _cuda(gt)
        w = np.linspace(0.25, 2.0, images).astype(np.float32)   # all different
        d = pred.astype(np.float64) - gt
        for kind in ("l1", "l2"):
            want_v = (np.abs(d) if kind == "l1" else d * d).mean(1)
            val, grad = loss.pixel_value_and_grad(p, g, kind, per_image=True)
            live = want_v != 0                                   # (n == 1 and x == y)
            np.testing.assert_allclose(val.cpu().numpy()[live], want_v[live], rtol=1e-5, err_msg=f"{kind} {images} x {n}")
            assert np.all(val.cpu().numpy()[~live] == 0)
            assert_every_element(grad.cpu().numpy(), pixel_want(kind, pred, gt, np.ones(images)), kind, f"{kind} {images} x {n} NULL")
            del grad
            got = _pixel_backward(kind, p, g, images, n, _cuda(w), 1).cpu().numpy()
            assert_every_element(got, pixel_want(kind, pred, gt, w), kind, f"{kind} {images} x {n} per-image upstream")
            got = _pixel_backward(kind, p, g, images, n, _cuda([0.6875]), 0).cpu().numpy()
            assert_every_element(got, pixel_want(kind, pred, gt, np.full(images, 0.6875)), kind, f"{kind} {images} x {n} scalar upstream")
        del p, g
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_pointwise_misaligned_views_every_element():
    """tests/test_loss_ext.py::test_gpu_l2_takes_a_misaligned_view element by element, the gradient buffer misaligned too and between canaries"""
    from youreditableavatar_amd import loss
    from youreditableavatar_amd.loss import _lib
    pred, gt = _inputs((3, 50, 70), seed=9)
    n = pred.size
    d = pred.astype(np.float64) - gt
    CANARY = 777.25
    st = torch.cuda.current_stream().cuda_stream
    for off_p, off_g, off_d in ((1, 0, 0), (0, 3, 0), (2, 2, 2), (0, 0, 1), (3, 1, 2), (0, 0, 0)):
        sp, sg = torch.zeros(n + 8).cuda(), torch.zeros(n + 8).cuda()
        p, g = sp[off_p:off_p + n], sg[off_g:off_g + n]
        p.copy_(torch.tensor(pred.reshape(-1))); g.copy_(torch.tensor(gt.reshape(-1)))
        assert p.data_ptr() % 16 == 4 * off_p and g.data_ptr() % 16 == 4 * off_g
        q = p.view(3, 50, 70).detach().requires_grad_(True)
        v = loss.l2_loss(q, g.view(3, 50, 70))
        v.backward()
        np.testing.assert_allclose(v.item(), (d * d).mean(), rtol=1e-5)
        assert_every_element(q.grad.cpu().numpy().reshape(-1), pixel_want("l2", pred.reshape(1, -1), gt.reshape(1, -1), 1.0)[0], "l2", f"l2_loss offsets {off_p, off_g}")
        for kind in ("l1", "l2"):
            for images in (1, 3):                               # (3 images of 3500 elements: n % 4 == 0, so alignment alone picks the path)
                per = n // images
                want = pixel_want(kind, pred.reshape(images, per), gt.reshape(images, per), 1.0).reshape(-1)
                sd = torch.full((n + 8,), CANARY).cuda()
                grad = sd[off_d:off_d + n]
                assert grad.data_ptr() % 16 == 4 * off_d
                _pixel_backward(kind, p, g, images, per, None, 0, grad=grad)
                assert_every_element(grad.cpu().numpy(), want, kind, f"backward {kind} offsets {off_p, off_g, off_d}")
                assert torch.all(sd[:off_d] == CANARY) and torch.all(sd[off_d + n:] == CANARY)
                sd.fill_(CANARY)
                nbytes = int(_lib.tgs_pixel_loss_workspace_bytes(images, per))
                ws, out = torch.empty(nbytes, dtype=torch.uint8).cuda(), torch.empty(images).cuda()
                assert _lib.tgs_pixel_loss(st, {"l1": 0, "l2": 1}[kind], images, per, p.data_ptr(), g.data_ptr(), out.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes) == 0
                assert_every_element(grad.cpu().numpy(), want, kind, f"value + gradient {kind} offsets {off_p, off_g, off_d}")
                e = (np.abs(d) if kind == "l1" else d * d).reshape(images, per).mean(1)
                np.testing.assert_allclose(out.cpu().numpy(), e, rtol=1e-5)
                assert torch.all(sd[:off_d] == CANARY) and torch.all(sd[off_d + n:] == CANARY)
        assert torch.all(sp[:off_p] == 0) and torch.all(sp[off_p + n:] == 0) and torch.all(sg[:off_g] == 0) and torch.all(sg[off_g + n:] == 0)
