"""GPU: the mask morphology and the blur (youreditableavatar_amd.mask_ops, csrc/tgs_mask_ops.hip) against the restatement (tests/mask_ops_ref.py): erode and
dilate bit for bit on shapes that straddle the 64-lane and the tile edges, every dtype, one and three channels, a non-contiguous view, two runs; the blur
under the derived bar of 2^-23 relative against float64, a constant image, and the exact support of the stage's dilate-then-blur chain.

The largest ratio |out - ref64| / (2^-23 |ref64|) seen on the MI355X over every blur case below: 0.4992, which is the one rounding to float (the double sums
are far below it)."""
import numpy as np
import pytest
import torch

from tests import mask_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 67), (67, 1), (63, 65), (130, 257)]
KERNELS = [1, 2, 3, 5, 20, 21, 30, 64, (2, 20)]
BAR = 2.0 ** -23
_ref = {}


def content(shape, C, kind):
    """the test images, by name: the same arrays every time"""
    H, W = shape
    full = (H, W) if C == 1 else (H, W, C)
    rng = np.random.default_rng(H * 1000 + W * 10 + C)
    if kind == "binary":                                                        # a random binary mask at 30 % density
        return (rng.random(full) < 0.3).astype(np.uint8) * 255
    if kind == "bytes":                                                         # a random uint8 image
        return rng.integers(0, 256, full, dtype=np.uint8)
    img = np.zeros(full, np.uint8)                                              # single pixels in all four corners and at columns 63 and 64
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 63), (H // 2, 64)):
        if x < W:
            img[y, x] = 255
    return img


def reference(op, shape, C, kind, kernel, as_dtype):
    key = (op, shape, C, kind, kernel, as_dtype)
    if key not in _ref:
        img = content(shape, C, kind)
        img = img > 0 if as_dtype == "bool" else img.astype(np.float32) / 4 - 17 if as_dtype == "float32" else img
        _ref[key] = (img, (R.erode if op == "erode" else R.dilate)(img, kernel))
    return _ref[key]


@pytest.mark.parametrize("kernel", KERNELS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_erode_and_dilate_equal_the_restatement(shape, kernel):
    from youreditableavatar_amd import mask_ops as mo
    cases = [(1, "binary", "uint8"), (1, "bytes", "uint8"), (1, "corners", "uint8"), (1, "binary", "bool"), (1, "bytes", "float32"), (3, "bytes", "uint8"), (3, "binary", "bool"),
             (3, "corners", "float32")]
    for C, kind, as_dtype in cases:
        for op, fn in (("erode", mo.erode), ("dilate", mo.dilate)):
            img, want = reference(op, shape, C, kind, kernel, as_dtype)
            t = torch.from_numpy(img).to(DEV)
            got = fn(t, kernel)
            assert got.shape == t.shape and got.dtype == t.dtype and got.device == t.device
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (op, C, kind, as_dtype)               # bit-equal everywhere
            assert torch.equal(fn(t, kernel), got)                                                           # two runs


def test_kernel_argument_forms_views_and_streams():
    from youreditableavatar_amd import mask_ops as mo
    img = content((130, 257), 3, "bytes")
    t = torch.from_numpy(img).to(DEV)
    want = torch.from_numpy(R.dilate(img, 20))
    for kernel in (20, (20, 20), np.ones((20, 20), np.uint8), torch.ones(20, 20, dtype=torch.uint8), torch.ones(20, 20, device=DEV)):
        assert torch.equal(mo.dilate(t, kernel).cpu(), want)
    assert torch.equal(mo.erode(t, np.ones((2, 5), np.uint8)).cpu(), torch.from_numpy(R.erode(img, (2, 5))))
    # non-contiguous views: every second row and column, a channel slice, a transposed image, a [H,W,1] slice as the stage makes with [:, :, :1]
    for view, ref in ((t[::2, 1::2], img[::2, 1::2]), (t[:, :, 1], img[:, :, 1]), (t[:, :, 0].t(), img[:, :, 0].T), (t[:, :, :1], img[:, :, :1]), (t.flip(0), img[::-1])):
        for kernel in (5, (2, 20)):
            assert torch.equal(mo.dilate(view, kernel).cpu(), torch.from_numpy(R.dilate(np.ascontiguousarray(ref), kernel)))
            assert torch.equal(mo.erode(view, kernel).cpu(), torch.from_numpy(R.erode(np.ascontiguousarray(ref), kernel)))
    for C in (2, 4):
        im = content((63, 65), C, "bytes")
        assert torch.equal(mo.erode(torch.from_numpy(im).to(DEV), 30).cpu(), torch.from_numpy(R.erode(im, 30)))
    assert mo.dilate(torch.zeros(0, 5, dtype=torch.uint8, device=DEV), 3).shape == (0, 5)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):                                               # a non-default stream
        got = mo.dilate(t, 20)
        blurred = mo.gaussian_blur(t[:, :, 0].float(), (21, 21))
    side.synchronize()
    assert torch.equal(got.cpu(), want) and torch.equal(blurred, mo.gaussian_blur(t[:, :, 0].float(), (21, 21)))


BLUR_SHAPES = [(11, 11), (33, 70), (130, 257)]
BLUR_KSIZES = [((3, 3), 0.0), ((21, 21), 0.0), ((5, 21), 0.0), ((21, 5), 0.0), ((21, 21), 2.0)]


@pytest.mark.parametrize("ksize,sigma", BLUR_KSIZES, ids=str)
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=str)
def test_blur_within_one_float_rounding_of_float64(shape, ksize, sigma):
    from youreditableavatar_amd import mask_ops as mo
    H, W = shape
    rng = np.random.default_rng(H + W)
    for img in (rng.random(shape, dtype=np.float32) * 255, (rng.random((H, W, 3)) < 0.3).astype(np.float32), np.add.outer(np.arange(H), np.arange(W)).astype(np.float32) / 7):        # (no negative values: the bar's derivation has no cancellation in it)
        want = R.gaussian_blur(img, ksize, sigma)
        t = torch.from_numpy(img).to(DEV)
        got = mo.gaussian_blur(t, ksize, sigma)
        assert got.shape == t.shape and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        nz = want != 0
        ratio = float((err[nz] / (BAR * np.abs(want[nz]))).max()) if nz.any() else 0.0
        print(f"blur {shape} {ksize} sigma {sigma}: largest |out - ref64| / (2^-23 |ref64|) = {ratio:.4f}")
        assert (err <= BAR * np.abs(want)).all(), ratio                         # |out - ref64| <= 2^-23 |ref64| per pixel
        assert torch.equal(mo.gaussian_blur(t, ksize, sigma), got)              # two runs
    for value in (1.0, 255.0, 0.3):                                             # a constant image stays within the bar of the constant
        const = mo.gaussian_blur(torch.full(shape, value, device=DEV), ksize, sigma).cpu().numpy().astype(np.float64)
        assert (np.abs(const - np.float32(value)) <= BAR * abs(float(np.float32(value)))).all()


@pytest.mark.parametrize("value", [1.0, 255.0])
def test_the_support_of_dilate_then_blur_is_exact(value):
    from youreditableavatar_amd import mask_ops as mo
    for shape, density in (((130, 257), 0.001), ((63, 65), 0.002), ((33, 70), 0.3)):
        m = (np.random.default_rng(7).random(shape) < density).astype(np.float32) * value
        m[0, 0] = m[-1, -1] = value
        t = torch.from_numpy(m).to(DEV)
        support = mo.gaussian_blur(mo.dilate(t, 20), (21, 21)) > 0
        want = R.morph(m, None, np.maximum, range(-20, 20), range(-20, 20)) > 0          # the dilation with offsets [-20, +19] in both axes
        assert torch.equal(support.cpu(), torch.from_numpy(want))
    # the chain of prepare_mask_proj on a uint8 mask: erode 2 -> dilate 20 -> float -> blur 21 -> > 0
    mask = content((130, 257), 3, "binary")
    t = torch.from_numpy(mask).to(DEV)
    got = mo.gaussian_blur(mo.dilate(mo.erode(t, np.ones((2, 2), np.uint8)), np.ones((20, 20), np.uint8)).float(), (21, 21), 0) > 0
    want = R.morph(R.erode(mask, 2), None, np.maximum, range(-20, 20), range(-20, 20)) > 0
    assert torch.equal(got.cpu(), torch.from_numpy(want))
