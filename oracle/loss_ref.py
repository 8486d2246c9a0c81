"""TEST INFRASTRUCTURE ONLY -- torch restatement of the reference's photometric loss (never imported by the product).

Pinned: tests/golden/ref_loss_fixture.npz holds outputs and autograd gradients of the reference's own
`utils/loss_utils.py` (l1_loss :17-18, ssim :39-63) imported in the build container (tests/make_ref_loss_fixture.py).

    loss = (1 - dssim_factor) * l1_loss(pred, gt) + dssim_factor * (1 - ssim(pred, gt))
(Edit_core/tetgs_texture/refine.py:245-247, refine_3dgs.py:277-279, paint_2dgs.py:345-347; dssim_factor = 0.2).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def gaussian_window(window_size: int = 11, sigma: float = 1.5, dtype=torch.float32) -> torch.Tensor:
    """loss_utils.py:23-25: normalised 1-D Gaussian (computed in Python doubles, stored as fp32 like torch.Tensor([...]))."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return (g / g.sum()).to(dtype)


def ssim_map(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    """loss_utils.py:27-58 for [C,H,W] or [B,C,H,W] images: zero-padded depthwise 11x11 Gaussian statistics."""
    C = img1.size(-3)
    if C == 1:
        # One channel goes through the depthwise convolution as the first of two channels: the same function (groups = C keeps the
        # channels apart), computed by the kernel the three-channel cases use.  With groups = 1 the CPU backend picks another kernel whose
        # fp32 backward depends on the CPU (fixture case c: 0, 7e-8 and 7e-3 rel-L2 on three x86 machines); the depthwise route reproduces
        # all four fixture cases bit for bit.
        z1, z2 = torch.zeros_like(img1), torch.zeros_like(img2)
        return ssim_map(torch.cat([img1, z1], -3), torch.cat([img2, z2], -3), window_size)[..., :1, :, :]
    w1 = gaussian_window(window_size, 1.5, torch.float32).unsqueeze(1)
    w2 = w1.mm(w1.t()).float().to(img1.dtype)                 # the reference forms the 2-D window in fp32 (:29)
    window = w2.unsqueeze(0).unsqueeze(0).expand(C, 1, window_size, window_size).contiguous().to(img1.device)
    conv = lambda x: F.conv2d(x, window, padding=window_size // 2, groups=C)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def ssim(img1, img2, window_size: int = 11):
    return ssim_map(img1, img2, window_size).mean()


def l1_loss(a, b):
    return torch.abs(a - b).mean()


def l1_ssim_loss(pred, gt, dssim_factor: float = 0.2):
    return (1.0 - dssim_factor) * l1_loss(pred, gt) + dssim_factor * (1.0 - ssim(pred, gt))


# ------------------------------------------------------------------------------------------------------------------------------------
# The pixel-by-pixel tests of tests/test_loss_pixelwise.py: the reference evaluated image by image in a chosen precision, an fp32
# restatement of the formulation the HIP kernels use (numpy; not the kernel), and the per-pixel judge.
# ------------------------------------------------------------------------------------------------------------------------------------
PIXEL_M = 4.0               # the kernel may sit this many times the reference's own local fp32 error from float64 ...
PIXEL_FLOOR = 2.0 ** -20    # ... or this fraction of the largest gradient element, where that error happens to be ~0


def _as_images(a: np.ndarray) -> np.ndarray:
    """[C,H,W] is one image: -> [B,C,H,W]"""
    a = np.asarray(a)
    return a[None] if a.ndim == 3 else a


def reference_value_and_grad(pred, gt, dssim_factor: float, dtype=torch.float64, upstream=None, per_image: bool = False):
    """l1_ssim_loss above by autograd in `dtype` on the CPU -> (out, grad) as float64 numpy arrays.
    per_image=False: out = [loss, ssim, l1] of the whole tensor, grad = upstream (a scalar, default 1) * d loss / d pred.
    per_image=True:  out = [B,3], grad = d (sum_b upstream[b] * loss_b) / d pred (upstream a scalar or one weight per image).
    Evaluated image by image -- the whole-tensor loss is the mean of the per-image losses of equally sized images -- so that the float64 graph
    of a 1080p batch stays one image large."""
    P, G = _as_images(pred), _as_images(gt)
    B = P.shape[0]
    up = np.broadcast_to(np.asarray(1.0 if upstream is None else upstream, np.float64), (B,)) * (1.0 if per_image else 1.0 / B)
    outs, grads = [], []
    for b in range(B):
        p = torch.tensor(P[b], dtype=dtype, requires_grad=True)
        g = torch.tensor(G[b], dtype=dtype)
        l1, s = l1_loss(p, g), ssim(p, g)
        loss = (1.0 - dssim_factor) * l1 + dssim_factor * (1.0 - s)
        (d,) = torch.autograd.grad(loss * float(up[b]), p)
        outs.append([loss.item(), s.item(), l1.item()])
        grads.append(d.double().numpy())
    outs = np.array(outs, np.float64)
    return (outs if per_image else outs.mean(0)), np.stack(grads).reshape(np.asarray(pred).shape)


def _window_pass(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """zero-padded separable 11-tap window over the last two axes in fp32, one rounding per product and per sum (no FMA): along the row from
    the tap furthest left, then down the column from the top row -- the order in which the kernels' sums travel"""
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-1] + (W + 10,), np.float32)
    p[..., 5:5 + W] = a
    h = w[10] * p[..., 0:W]
    for j in range(9, -1, -1):
        h = h + w[j] * p[..., 10 - j:10 - j + W]
    q = np.zeros(a.shape[:-2] + (H + 10, W), np.float32)
    q[..., 5:5 + H, :] = h
    v = w[0] * q[..., 0:H, :]
    for k in range(1, 11):
        v = v + w[k] * q[..., k:k + H, :]
    return v


def kernel_formulation_fp32(pred, gt, dssim_factor: float, upstream=None, per_image: bool = False):
    """What csrc/tgs_loss.hip computes, restated in fp32 numpy: FOUR windowed maps (x, y, x^2 + y^2, xy), D2 = (SS - mu1^2 - mu2^2) + C2, the
    three derivative maps and the adjoint window over them.  Exact division where the kernel has v_rcp_f32 and no contraction, so this is
    the formulation's own rounding, not the kernel's.  Same arguments and results as reference_value_and_grad (out in float64: the
    kernels reduce their partial sums in double)."""
    f32 = np.float32
    P, G = _as_images(pred).astype(f32), _as_images(gt).astype(f32)
    B = P.shape[0]
    w = gaussian_window().numpy()
    count = P[0].size * (1 if per_image else B)
    m1, m2, SS, XY = (_window_pass(a, w) for a in (P, G, P * P + G * G, P * G))
    C1, C2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
    m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
    s12 = XY - m12
    N1, N2, D1, D2 = f32(2) * m12 + C1, f32(2) * s12 + C2, m11 + m22 + C1, (SS - m11 - m22) + C2
    iD1, iD2 = f32(1) / D1, f32(1) / D2
    q = iD1 * iD2
    smap = N1 * N2 * q
    dM1 = f32(2) * q * (m2 * (N2 - N1) - m1 * smap * (D2 - D1))
    dX2 = -smap * iD2
    dXY = f32(2) * N1 * q
    A, Bm, Cm = (_window_pass(a, w) for a in (dM1, dX2, dXY))
    gs, gl = f32(-float(dssim_factor) / count), f32((1.0 - float(dssim_factor)) / count)
    up = np.broadcast_to(np.asarray(1.0 if upstream is None else upstream, f32), (B,)).reshape(B, 1, 1, 1)
    d = P - G
    grad = (gl * up) * np.sign(d) + (gs * up) * (A + f32(2) * P * Bm + G * Cm)
    s = smap.astype(np.float64).mean((1, 2, 3))
    l1 = np.abs(d).astype(np.float64).mean((1, 2, 3))
    outs = np.stack([(1.0 - dssim_factor) * l1 + dssim_factor * (1.0 - s), s, l1], 1)
    return (outs if per_image else outs.mean(0)), grad.reshape(np.asarray(pred).shape)


def local_envelope(err: np.ndarray) -> np.ndarray:
    """max of `err` over the 21 x 21 pixels around each pixel of its own plane (an 11 x 11 window and its adjoint reach that far)"""
    e = torch.tensor(np.ascontiguousarray(err, dtype=np.float64))
    shape = e.shape
    e = F.max_pool2d(e.reshape(-1, 1, shape[-2], shape[-1]), kernel_size=21, stride=1, padding=10)
    return e.reshape(shape).numpy()


def pixel_bars(want: np.ndarray, ref32: np.ndarray, M: float = PIXEL_M, floor: float = PIXEL_FLOOR) -> np.ndarray:
    """per pixel: max(M * env, floor * max|want|), env = the reference's own fp32 error |ref32 - want| at its worst within reach"""
    want = np.asarray(want, np.float64)
    return np.maximum(M * local_envelope(np.abs(np.asarray(ref32, np.float64) - want)), floor * np.abs(want).max())


def _rel_l2(x, ref) -> float:
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-12))


def judge(got, want, ref32, bars=None, M: float = PIXEL_M, floor: float = PIXEL_FLOOR) -> dict:
    """Every pixel of `got` against `want` (float64) under pixel_bars; the whole tensor under max(1e-5, 2 eta), eta = rel-L2 of ref32 from want.
    -> worst (the largest |got - want| / bar; passes iff <= 1 and every element finite), over (pixels above their bar), where (index of the
    worst pixel), rel_l2, eta, rel_l2_bar.  No pixel is left out."""
    got, want, ref32 = (np.asarray(a, np.float64) for a in (got, want, ref32))
    assert got.shape == want.shape == ref32.shape, (got.shape, want.shape, ref32.shape)
    bars = pixel_bars(want, ref32, M, floor) if bars is None else bars
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / bars)             # (an exact element passes a bar of 0: want == 0 everywhere)
    ratio[~np.isfinite(ratio)] = np.inf
    eta = _rel_l2(ref32, want)
    return {"worst": float(ratio.max()), "over": int((ratio > 1.0).sum()), "where": [int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape)],
            "rel_l2": _rel_l2(got, want), "eta": eta, "rel_l2_bar": max(1e-5, 2.0 * eta), "pixels": int(ratio.size)}


def passes(rep: dict) -> bool:
    return rep["worst"] <= 1.0 and rep["rel_l2"] <= rep["rel_l2_bar"]
