"""GPU: the mask morphology and the blur (csrc/tgs_mask_ops.hip) at the launch shapes tests/test_gpu_mask_ops.py never reaches.

Morphology, bit for bit against ``R.erode`` / ``R.dilate``, erode and dilate, two runs:
  - C = 4 and C = 2 with the kernels 64, (64, 1), (1, 64), 63 and 2 on (17, 65), (33, 129), (16, 64): for C = 4 a line has 260, 516 and 256 elements (across
    one seam of the 256-element row tile, across two, exactly one tile) and H lies across and on the 16-line seam.  C = 4 with kw = 64 stages 256 + 63 * 4 =
    508 elements, all that the row pass's LDS array is declared for.
  - images smaller than the rectangle's reach that still cross a seam: (3, 300), (300, 3), (1, 513), (513, 1)
  - float images drawn from +-inf, +-FLT_MAX, +-FLT_MIN, six subnormals of both signs and +-1 (no zero: the sign of a zero is not part of the rule):
    the exact min / max, compared as int32 words
  - every second column of a (33, 258, 4) tensor, which is the row pass's strided index expression at C = 4, and its flip

Blur, |out - ref64| <= 2^-23 |ref64| per pixel against ``R.gaussian_blur`` on non-negative images (the bar the sibling module derives), every case twice:
  - ksize 1, 7, 9, 31, (31, 1), (1, 31) at sigma 0 and 3, 5, 7, 31 at sigma 1.5 (the fixed tables must not be used there), C = 1, 2, 4, on (16, 16), the
    smallest legal image at k = 31 where both reflections fold into the same line, (16, 300) and (130, 65); constant images
  - strided inputs: a channel slice, a transpose, a flip, every second row and column, a [H,W,1] slice
  - an impulse at each corner and on both sides of the column seam of a (40, 300) image at k = 31 against the outer product of the reflected weight rows,
    the reflection written as a fold of positions and not as ``R.reflect101``

The largest ratio |out - ref64| / (2^-23 |ref64|) seen on the MI355X over the 277 blur cases below: 0.4999 ((16, 300), C = 2 and 4, the binary
mask, ksize (5, 5) at sigma 1.5), which is the one rounding to float; the sibling module reports 0.4992."""
import numpy as np
import pytest
import torch

from tests import mask_ops_ref as R
from tests.test_gpu_mask_ops import BAR, DEV, content, reference

pytestmark = pytest.mark.gpu
OPS = ("erode", "dilate")


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    """shape, dtype and every bit: a float as its int32 word"""
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    return torch.equal(got.view(torch.int32), want.view(torch.int32)) if got.dtype == torch.float32 else torch.equal(got, want)


def check_morph(img: np.ndarray, kernel, what, view=None):
    """erode and dilate of ``view`` (default: the whole image on the device) against the restatement on ``img``, two runs"""
    from youreditableavatar_amd import mask_ops as mo
    t = torch.from_numpy(img).to(DEV) if view is None else view
    for op, fn, ref in (("erode", mo.erode, R.erode), ("dilate", mo.dilate, R.dilate)):
        got = fn(t, kernel)
        assert got.device == t.device and same_bits(got, ref(img, kernel)), (op, kernel) + what
        assert same_bits(fn(t, kernel), got.cpu().numpy()), (op, kernel, "second run") + what


@pytest.mark.parametrize("C", [4, 2])
@pytest.mark.parametrize("shape", [(17, 65), (33, 129), (16, 64)], ids=str)
def test_wide_kernels_on_two_and_four_channels(shape, C):
    from youreditableavatar_amd import mask_ops as mo
    for kernel in (64, (64, 1), (1, 64), 63, 2):
        for kind, as_dtype in (("bytes", "uint8"), ("binary", "bool"), ("bytes", "float32")):
            for op in OPS:
                img, want = reference(op, shape, C, kind, kernel, as_dtype)
                t = torch.from_numpy(img).to(DEV)
                got = getattr(mo, op)(t, kernel)
                assert same_bits(got, want), (op, kernel, as_dtype)
                assert torch.equal(getattr(mo, op)(t, kernel), got), (op, kernel, as_dtype, "second run")


@pytest.mark.parametrize("shape", [(3, 300), (300, 3), (1, 513), (513, 1)], ids=str)
def test_images_smaller_than_the_reach_across_a_seam(shape):
    for C in (1, 4):
        img = content(shape, C, "bytes")
        for kernel in (64, (64, 2), (2, 64)):
            check_morph(img, kernel, (shape, C, "uint8"))
            check_morph(img.astype(np.float32) / 4 - 17, kernel, (shape, C, "float32"))
            check_morph(content(shape, C, "binary") > 0, kernel, (shape, C, "bool"))


SUBNORMALS = [np.float32(2.0 ** -149) * m for m in (1, 2, 3, 0x400000, 0x7ffffe, 0x7fffff)]          # the least, its neighbours, the middle, the two largest


def special_floats(which):
    fi = np.finfo(np.float32)
    sub = np.array(SUBNORMALS, np.float32)
    assert len(set(sub.view(np.int32).tolist())) == 6 and (sub > 0).all() and (sub < fi.tiny).all()
    if which == "subnormals":
        return np.concatenate([sub, -sub])
    return np.concatenate([sub, -sub, np.array([np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, 1.0, -1.0], np.float32)])


@pytest.mark.parametrize("which", ["all", "subnormals"])
def test_float_min_and_max_are_exact_on_subnormals_and_infinities(which):
    values = special_floats(which)
    for shape, C in (((33, 129), 1), ((17, 65), 4)):
        full = shape if C == 1 else shape + (C,)
        img = values[np.random.default_rng(len(values) + C).integers(0, len(values), full)]
        assert img.dtype == np.float32 and not (img == 0).any() and len(np.unique(img.view(np.int32))) == len(values)
        for kernel in (2, 3, 5, (1, 64), 64):
            check_morph(img, kernel, (which, shape, C))


def test_strided_four_channel_source():
    wide = content((33, 258), 4, "bytes")
    for img in (wide, wide.astype(np.float32) / 4 - 17):
        t = torch.from_numpy(img).to(DEV)
        view = t[:, ::2]
        assert view.shape == (33, 129, 4) and view.stride() == (258 * 4, 8, 1)
        check_morph(np.ascontiguousarray(img[:, ::2]), 64, ("every second column", img.dtype), view)
        check_morph(np.ascontiguousarray(img[:, ::2][:, ::-1]), 64, ("every second column, flipped", img.dtype), view.flip(1))


# ---- the blur ----
def blur_images(shape, C):
    """the three non-negative images of the sibling module, with C channels: uniform in [0, 255), a 30 % binary mask, a ramp"""
    H, W = shape
    full = shape if C == 1 else shape + (C,)
    rng = np.random.default_rng(H + W + C)
    ramp = np.add.outer(np.arange(H), np.arange(W)).astype(np.float32) / 7
    return rng.random(full, dtype=np.float32) * 255, (rng.random(full) < 0.3).astype(np.float32), ramp if C == 1 else np.stack([ramp + c for c in range(C)], axis=2)


def check_blur(t: torch.Tensor, want: np.ndarray, ksize, sigma, what):
    """|out - want| <= 2^-23 |want| per pixel, the ratio printed first; two runs"""
    from youreditableavatar_amd import mask_ops as mo
    got = mo.gaussian_blur(t, ksize, sigma)
    assert got.shape == t.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    nz = want != 0
    ratio = float((err[nz] / (BAR * np.abs(want[nz]))).max()) if nz.any() else 0.0
    print(f"blur {what} {ksize} sigma {sigma}: largest |out - ref64| / (2^-23 |ref64|) = {ratio:.4f}")
    assert (err <= BAR * np.abs(want)).all(), (what, ratio)
    assert torch.equal(mo.gaussian_blur(t, ksize, sigma), got), what             # two runs


@pytest.mark.parametrize("ksize,sigma", [((1, 1), 0.0), ((7, 7), 0.0), ((9, 9), 0.0), ((31, 31), 0.0), ((31, 1), 0.0), ((1, 31), 0.0),
                                         ((3, 3), 1.5), ((5, 5), 1.5), ((7, 7), 1.5), ((31, 31), 1.5)], ids=str)
def test_blur_kernels_channels_and_the_smallest_image(ksize, sigma):
    from youreditableavatar_amd import mask_ops as mo
    for shape in ((16, 16), (16, 300), (130, 65)):
        for C in (1, 2, 4):
            for i, img in enumerate(blur_images(shape, C)):
                assert (img >= 0).all()
                check_blur(torch.from_numpy(img).to(DEV), R.gaussian_blur(img, ksize, sigma), ksize, sigma, (shape, C, i))
            full = shape if C == 1 else shape + (C,)
            for value in (1.0, 255.0, 0.3):                                     # a constant image stays within the bar of the constant
                const = mo.gaussian_blur(torch.full(full, value, device=DEV), ksize, sigma).cpu().numpy().astype(np.float64)
                assert (np.abs(const - np.float32(value)) <= BAR * abs(float(np.float32(value)))).all(), (shape, C, value)


@pytest.mark.parametrize("ksize,sigma", [((31, 31), 0.0), ((7, 7), 1.5), ((5, 21), 0.0)], ids=str)
def test_blur_of_strided_inputs(ksize, sigma):
    img = blur_images((40, 300), 4)[0]
    t = torch.from_numpy(img).to(DEV)
    views = {"channel slice": (t[:, :, 1], img[:, :, 1]), "transposed": (t[:, :, 0].t(), img[:, :, 0].T), "flipped": (t.flip(0), img[::-1]),
             "every second row and column": (t[::2, 1::2], img[::2, 1::2]), "[H,W,1] slice": (t[:, :, :1], img[:, :, :1])}
    for name, (view, ref) in views.items():
        if name != "flipped":
            assert not view.is_contiguous() or view.shape[-1] == 1
        check_blur(view, R.gaussian_blur(np.ascontiguousarray(ref), ksize, sigma), ksize, sigma, name)


def reflected_weights(w, n, at):
    """row[x] = the sum of the taps of ``w`` that, centred on x, land on position ``at`` of a line of n under BORDER_REFLECT_101: the line mirrored about its
    first and its last element without repeating them, written as a fold of the position"""
    r = len(w) // 2
    row = np.zeros(n)
    for x in range(n):
        for i in range(len(w)):
            p = x + i - r
            if p < 0:
                p = -p                                                          # ... 2 1 | 0 1 2 ...
            if p > n - 1:
                p = (n - 1) - (p - (n - 1))                                     # ... n-2 n-1 | n-2 n-3 ...
            if p == at:
                row[x] += w[i]
    return row


def test_blur_of_an_impulse_is_the_outer_product_of_the_reflected_weights():
    H, W, ksize = 40, 300, (31, 31)
    w = R.gaussian_kernel(31)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 255), (H // 2, 256)):
        img = np.zeros((H, W), np.float32)
        img[y, x] = 1.0
        want = np.outer(reflected_weights(w, H, y), reflected_weights(w, W, x))
        assert (want > 0).sum() == (16 if y in (0, H - 1) else 31) * (16 if x in (0, W - 1) else 31)                  # a corner's mirror image coincides with it: 16 lines, not 31
        check_blur(torch.from_numpy(img).to(DEV), want, ksize, 0.0, ("impulse", y, x))
