"""NumPy restatement of the rules of include/tgs_raster.h, "mask morphology and blur": naive loops over the offsets of the rectangle and over the taps.
The yardstick of youreditableavatar_amd.mask_ops; checked itself in tests/test_mask_ops_ref.py against hand cases and scipy.ndimage."""
import math

import numpy as np

SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625], 7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def kernel_size(kernel):
    return (int(kernel), int(kernel)) if np.isscalar(kernel) else (int(kernel[0]), int(kernel[1]))


def offsets(k):
    """the offsets of a k-wide rectangle with the default anchor k // 2: [-(k // 2), k - 1 - k // 2]"""
    a = k // 2
    return range(-a, k - a)


def morph(img, kernel, op, dy_range=None, dx_range=None):
    """op: np.minimum (erode) or np.maximum (dilate).  dst(y,x) = op over src(y+dy, x+dx), dy and dx over the rectangle's offsets; positions outside the
    image take no part.  [H,W] or [H,W,C]; channels are independent.  ``dy_range`` / ``dx_range`` replace the rectangle's offsets (the blur's support test)."""
    img = np.asarray(img)
    kh, kw = kernel_size(kernel) if kernel is not None else (0, 0)
    dys = list(dy_range if dy_range is not None else offsets(kh))
    dxs = list(dx_range if dx_range is not None else offsets(kw))
    H, W = img.shape[:2]
    out = img.copy()                                                            # (offset (0, 0) is always one of them)
    for dy in dys:
        for dx in dxs:
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)       # the destination pixels whose source (y + dy, x + dx) is inside
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] = op(out[y0:y1, x0:x1], img[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    return out


def erode(img, kernel):
    return morph(img, kernel, np.minimum)


def dilate(img, kernel):
    return morph(img, kernel, np.maximum)


def gaussian_kernel(k, sigma=0.0):
    """OpenCV's getGaussianKernel in float64"""
    if sigma <= 0 and k in SMALL_GAUSSIAN:
        return np.array(SMALL_GAUSSIAN[k], np.float64)
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    w = np.array([math.exp(-((i - k // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(k)], np.float64)
    return w / w.sum()


def reflect101(i, n):
    """index -1 -> 1, n -> n - 2"""
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def gaussian_blur(img, ksize, sigma=0.0):
    """float64: the row pass over the taps i = 0 .. kw - 1 in that order, then the column pass; ksize = (kw, kh); BORDER_REFLECT_101"""
    img = np.asarray(img, np.float64)
    kw, kh = int(ksize[0]), int(ksize[1])
    H, W = img.shape[:2]
    assert kw % 2 and kh % 2 and H > kh // 2 and W > kw // 2
    wx, wy = gaussian_kernel(kw, sigma), gaussian_kernel(kh, sigma)
    xs, ys = np.arange(W), np.arange(H)
    rows = np.zeros_like(img)
    for i in range(kw):
        rows += wx[i] * img[:, reflect101(xs + i - kw // 2, W)]
    out = np.zeros_like(img)
    for i in range(kh):
        out += wy[i] * rows[reflect101(ys + i - kh // 2, H)]
    return out
