"""CPU: the restatement of the mask morphology and the blur (tests/mask_ops_ref.py) checked three ways: the hand cases of include/tgs_raster.h, scipy's
rank filters with a constant border, and scipy's correlate1d with the mirrored border and the same weights."""
import numpy as np
import pytest

from tests import mask_ops_ref as R


def impulse(H=48, W=52, y=24, x=25, value=255, dtype=np.uint8):
    img = np.zeros((H, W), dtype)
    img[y, x] = value
    return img


@pytest.mark.parametrize("k,lo,hi", [(2, 0, 1), (5, -2, 2), (20, -9, 10), (1, 0, 0), (3, -1, 1), (64, -31, 32)])
def test_hand_cases_of_an_impulse(k, lo, hi):
    y, x = 24, 25
    want = np.zeros((48, 52), np.uint8)
    want[max(0, y + lo):y + hi + 1, max(0, x + lo):x + hi + 1] = 255
    assert np.array_equal(R.dilate(impulse(), k), want)                         # a set pixel at (y, x) sets (y + lo .. y + hi, x + lo .. x + hi)
    hole = 255 - impulse()
    assert np.array_equal(R.erode(hole, k), 255 - want)                         # erosion: the same with the zeros
    assert np.array_equal(R.erode(impulse(), 1), impulse()) and np.array_equal(R.dilate(impulse(), 1), impulse())


def test_offsets_borders_and_channels():
    assert list(R.offsets(2)) == [-1, 0] and list(R.offsets(5)) == [-2, -1, 0, 1, 2] and list(R.offsets(20)) == list(range(-10, 10)) and list(R.offsets(1)) == [0]
    # (dst(x) = max src(x + dx), dx in [-10, 9]: a set pixel at p reaches the x with p - x in [-10, 9], which is x - 9 .. x + 10 as the header says)
    img = np.full((5, 6), 200, np.uint8)
    assert np.array_equal(R.erode(img, 64), img) and np.array_equal(R.dilate(img, (64, 3)), img)          # a rectangle larger than the image; the border takes no part
    corner = np.zeros((4, 4), np.uint8)
    corner[0, 0] = corner[3, 3] = 9
    assert np.array_equal(R.dilate(corner, 2), np.array([[9, 9, 0, 0], [9, 9, 0, 0], [0, 0, 0, 0], [0, 0, 0, 9]], np.uint8))
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    out = R.dilate(rgb, (2, 20))
    for c in range(3):
        assert np.array_equal(out[..., c], R.dilate(rgb[..., c], (2, 20)))      # channels are independent
    assert R.dilate(rgb > 128, 3).dtype == bool and R.erode(rgb.astype(np.float32), 3).dtype == np.float32


@pytest.mark.parametrize("kernel", [1, 2, 3, 5, 20, 21, 30, 64, (2, 20), (20, 2)])
def test_against_scipy_rank_filters(kernel):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    kh, kw = R.kernel_size(kernel)
    for img in (rng.integers(0, 256, (37, 41), dtype=np.uint8), (rng.random((23, 70)) < 0.3).astype(np.uint8) * 255, impulse(30, 31, 0, 0), impulse(30, 31, 29, 30)):
        # scipy centres a window of size k at origin 0 on offsets [-(k // 2), k - 1 - k // 2]: the rectangle with the default anchor
        assert np.array_equal(R.dilate(img, kernel), ndi.maximum_filter(img, size=(kh, kw), mode="constant", cval=0))
        assert np.array_equal(R.erode(img, kernel), ndi.minimum_filter(img, size=(kh, kw), mode="constant", cval=255))


def test_gaussian_coefficients():
    assert np.array_equal(R.gaussian_kernel(3), [0.25, 0.5, 0.25]) and np.array_equal(R.gaussian_kernel(1), [1.0])
    assert np.array_equal(R.gaussian_kernel(5), [0.0625, 0.25, 0.375, 0.25, 0.0625])
    w = R.gaussian_kernel(21)                                                   # sigma = 0.3 * (10 - 1) + 0.8 = 3.5
    ref = np.exp(-(np.arange(21) - 10.0) ** 2 / (2 * 3.5 ** 2))
    assert np.allclose(w, ref / ref.sum(), rtol=1e-14, atol=0) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    assert 3.6e-6 < w[0] * w[0] < 3.8e-6                                        # the smallest weight product of a (21, 21) blur: the support is exact in float32
    assert np.allclose(R.gaussian_kernel(21, 2.0), np.exp(-(np.arange(21) - 10.0) ** 2 / 8) / np.exp(-(np.arange(21) - 10.0) ** 2 / 8).sum(), rtol=1e-14)
    assert list(R.reflect101(np.array([-2, -1, 0, 4, 5, 6]), 5)) == [2, 1, 0, 4, 3, 2]


@pytest.mark.parametrize("ksize,sigma", [((3, 3), 0.0), ((21, 21), 0.0), ((5, 21), 0.0), ((21, 5), 0.0), ((21, 21), 2.0)])
def test_blur_against_scipy_correlate1d(ksize, sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    for shape in ((11, 11), (33, 70), (16, 19, 3)):
        img = rng.random(shape)
        rows = ndi.correlate1d(img, R.gaussian_kernel(ksize[0], sigma), axis=1, mode="mirror")
        want = ndi.correlate1d(rows, R.gaussian_kernel(ksize[1], sigma), axis=0, mode="mirror")
        got = R.gaussian_blur(img, ksize, sigma)
        assert np.allclose(got, want, rtol=1e-13, atol=0)
    got = R.gaussian_blur(np.full((12, 13), 7.0), ksize, sigma)
    assert np.allclose(got, 7.0, rtol=1e-14)


def test_blur_support_of_an_impulse():
    blurred = R.gaussian_blur(impulse(64, 64, 30, 31, 1.0, np.float64), (21, 21))
    assert int((blurred > 0).sum()) == 441 and (blurred[20:41, 21:42] > 0).all()
    assert (blurred.astype(np.float32) > 0).sum() == 441                        # the smallest value survives the rounding to float32
    m = (np.random.default_rng(3).random((50, 60)) < 0.02).astype(np.float64)
    support = R.gaussian_blur(R.dilate(m, 20), (21, 21)) > 0
    assert np.array_equal(support, R.morph(m, None, np.maximum, range(-20, 20), range(-20, 20)) > 0)       # offsets [-20, +19] in both axes


# ---- what the cases of tests/test_gpu_mask_ops_launch.py rest on ----
def test_sigma_above_zero_never_takes_the_table():
    from youreditableavatar_amd import mask_ops
    for k in (3, 5, 7, 31):
        mine, ref = mask_ops.gaussian_kernel(k, 1.5), R.gaussian_kernel(k, 1.5)
        assert mine.dtype == np.float64 and np.array_equal(mine, ref) and abs(mine.sum() - 1) < 1e-15
        exact = np.exp(-(np.arange(k) - k // 2) ** 2 / 4.5)
        assert np.allclose(mine, exact / exact.sum(), rtol=1e-14, atol=0)
        if k in R.SMALL_GAUSSIAN:
            assert not np.array_equal(mine, R.SMALL_GAUSSIAN[k]) and np.array_equal(mask_ops.gaussian_kernel(k, 0.0), R.SMALL_GAUSSIAN[k])
    assert np.array_equal(mask_ops.gaussian_kernel(9), R.gaussian_kernel(9)) and np.array_equal(mask_ops.gaussian_kernel(31), R.gaussian_kernel(31))
    w = R.gaussian_kernel(31)                                                   # sigma = 0.3 * (15 - 1) + 0.8 = 5
    assert np.allclose(w, np.exp(-(np.arange(31) - 15.0) ** 2 / 50) / np.exp(-(np.arange(31) - 15.0) ** 2 / 50).sum(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("ksize,sigma", [((31, 31), 0.0), ((31, 1), 0.0), ((1, 31), 0.0), ((9, 9), 0.0), ((7, 7), 1.5), ((31, 31), 1.5)])
def test_blur_of_the_smallest_image_and_of_two_and_four_channels_against_scipy(ksize, sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(4)
    for shape in ((16, 16), (16, 16, 2), (16, 300, 4), (130, 65, 2)):           # 16: the smallest legal line at k = 31, folded at both ends
        img = rng.random(shape)
        rows = ndi.correlate1d(img, R.gaussian_kernel(ksize[0], sigma), axis=1, mode="mirror")
        want = ndi.correlate1d(rows, R.gaussian_kernel(ksize[1], sigma), axis=0, mode="mirror")
        assert np.allclose(R.gaussian_blur(img, ksize, sigma), want, rtol=1e-13, atol=0)


def test_min_and_max_of_subnormals_and_infinities_are_exact():
    pytest.importorskip("torch")
    from tests.test_gpu_mask_ops_launch import special_floats
    values = special_floats("all")
    assert len(values) == 20 and len(set(values.view(np.int32).tolist())) == 20 and not (values == 0).any()
    img = values[np.random.default_rng(5).integers(0, 20, (9, 11))]
    for k, ref, pick in ((3, R.erode, min), (2, R.dilate, max)):
        got = ref(img, k)
        for y in range(9):
            for x in range(11):                                                 # Python floats: every float32 exactly, compared exactly
                window = [float(img[yy, xx]) for yy in range(max(0, y - k // 2), min(9, y + k - k // 2)) for xx in range(max(0, x - k // 2), min(11, x + k - k // 2))]
                assert float(got[y, x]) == pick(window) and got[y, x].view(np.int32) in img.view(np.int32)
