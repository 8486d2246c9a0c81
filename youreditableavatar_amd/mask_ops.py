"""The image operations of the painting stage on the device: ``erode``, ``dilate`` and ``gaussian_blur`` with the call shapes of ``cv2.erode``, ``cv2.dilate``
and ``cv2.GaussianBlur`` as ``prepare_mask_proj`` (``tetgs_inpainter/mask_mesh_0822.py`` :153-207) and ``normal_based_inpaint`` (``inpaint_utils.py`` :27-39)
call them.  The reference writes the antialiased mask to a PNG, reads it back, runs cv2 on the host and copies the result to the device; here the mask stays
where ``antialias`` left it, and every call is enqueued on the current stream with no host copy and no read-back.

The kernels are ``csrc/tgs_mask_ops.hip``; the rules are written down in include/tgs_raster.h, "mask morphology and blur", and restated in
tests/mask_ops_ref.py.  HIP tensors only: there is no CPU path.  An image is ``[H,W]`` or ``[H,W,C]`` with ``C <= 4``, cv2's layout, any strides.
All decisions are exact min / max or a fixed-order double sum rounded once: two runs give the same bits.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import _host
from ._host import _I, _L, _P, _Z, guard as _guard, need_device as _need_device, ok as _ok, raw_stream as _raw_stream, workspace as _workspace

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_maskops_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "tgs_maskops_morph": (_I, [_P, _I, _I, _I, _I, _I, _P, _L, _L, _L, _I, _I, _P, _P, _Z]),
    "tgs_maskops_blur": (_I, [_P, _I, _I, _I, _P, _L, _L, _L, _I, _I, _P, _P, _P, _P, _Z]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_KERNEL = 64                    # erode / dilate: 1 <= kh, kw <= 64
MAX_BLUR_KERNEL = 31               # gaussian_blur: odd, <= 31
MAX_CHANNELS = 4
_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625], 7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def _kernel_size(kernel) -> Tuple[int, int]:
    """an int ``k``, a pair ``(kh, kw)``, or an all-ones array / tensor of that shape -> (kh, kw); a kernel that is a device tensor is read back to see that
    it is all ones (the call sites pass ``np.ones``: nothing is read back for those)"""
    if isinstance(kernel, (torch.Tensor, np.ndarray)):
        k = kernel.detach().cpu().numpy() if isinstance(kernel, torch.Tensor) else kernel
        if k.ndim != 2 or k.size == 0:
            raise RuntimeError(f"expected a structuring element of shape [kh,kw], got {tuple(k.shape)}")
        if not (k == 1).all():
            raise RuntimeError("only the full rectangle is served: the structuring element must be all ones (np.ones((kh, kw), np.uint8))")
        kh, kw = int(k.shape[0]), int(k.shape[1])
    elif isinstance(kernel, (int, np.integer)) and not isinstance(kernel, bool):
        kh = kw = int(kernel)
    elif isinstance(kernel, (tuple, list)) and len(kernel) == 2 and all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in kernel):
        kh, kw = int(kernel[0]), int(kernel[1])
    else:
        raise RuntimeError(f"kernel is an int k, a pair (kh, kw) or an all-ones array of that shape, got {kernel!r}")
    if not (1 <= kh <= MAX_KERNEL and 1 <= kw <= MAX_KERNEL):
        raise RuntimeError(f"1 <= kh, kw <= {MAX_KERNEL} is required, got ({kh}, {kw})")
    return kh, kw


def _image(name: str, img, dtypes) -> Tuple[int, int, int]:
    if not isinstance(img, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if img.dtype not in dtypes:
        if img.dtype == torch.uint8 and torch.float32 in dtypes:
            raise RuntimeError("gaussian_blur serves float32 only: a uint8 image is not served, convert it first (the reference's calls do, with .astype(np.float32))")
        raise RuntimeError(f"expected {name} of dtype {' / '.join(str(d).replace('torch.', '') for d in dtypes)}, got {img.dtype}")
    if img.dim() not in (2, 3):
        raise RuntimeError(f"expected {name} of shape [H,W] or [H,W,C], got {tuple(img.shape)}")
    C = int(img.shape[2]) if img.dim() == 3 else 1
    if not 1 <= C <= MAX_CHANNELS:
        raise RuntimeError(f"1 <= C <= {MAX_CHANNELS} is required, got C = {C}")
    return int(img.shape[0]), int(img.shape[1]), C


def _strides(img: torch.Tensor) -> Tuple[int, int, int]:
    return img.stride(0), img.stride(1), (img.stride(2) if img.dim() == 3 else 0)


def _morph(op: int, img, kernel) -> torch.Tensor:
    H, W, C = _image("img", img, (torch.uint8, torch.bool, torch.float32))
    kh, kw = _kernel_size(kernel)
    dev = _need_device("mask_ops", img=img)
    src = img.detach()
    src = src.view(torch.uint8) if src.dtype == torch.bool else src
    out = torch.empty(tuple(img.shape), dtype=src.dtype, device=dev)
    if H * W:
        is_float = src.dtype == torch.float32
        ws, nbytes = _workspace(_lib.tgs_maskops_workspace_bytes(H, W, C, 4 if is_float else 1), dev)
        with _guard(dev):
            _ok(_lib.tgs_maskops_morph(_raw_stream(dev.index), op, int(is_float), H, W, C, src.data_ptr(), *_strides(src), kh, kw, out.data_ptr(), ws.data_ptr(), nbytes))
    return out.view(torch.bool) if img.dtype == torch.bool else out


def erode(img: torch.Tensor, kernel) -> torch.Tensor:
    """``cv2.erode(img, kernel)``: ``img`` [H,W] or [H,W,C], ``C <= 4``, uint8, bool or float32, any strides -> the same shape and dtype.  ``kernel`` is an int
    ``k``, a pair ``(kh, kw)`` or an all-ones array or tensor of that shape, ``1 <= kh, kw <= 64``.  Default anchor ``k // 2`` and default border:
    ``dst(y,x) = min src(y+dy, x+dx)`` over ``dy`` in ``[-(kh//2), kh-1-kh//2]``, ``dx`` likewise; positions outside the image take no part.  Channels are
    independent.  A float NaN: not defined."""
    return _morph(0, img, kernel)


def dilate(img: torch.Tensor, kernel) -> torch.Tensor:
    """``cv2.dilate(img, kernel)``: as ``erode`` with the max.  A 2x2 dilation of one set pixel at (y, x) sets (y..y+1, x..x+1); a 20x20 one sets x-9..x+10.
    A float NaN: not defined."""
    return _morph(1, img, kernel)


def gaussian_kernel(k: int, sigma: float = 0.0) -> np.ndarray:
    """OpenCV's ``getGaussianKernel(k, sigma)`` in float64: for ``sigma <= 0`` the fixed tables of k = 1, 3, 5, 7, else ``sigma = 0.3*((k-1)*0.5 - 1) + 0.8``;
    ``exp(-(i - k//2)^2 / (2 sigma^2))`` normalised to sum 1."""
    if sigma <= 0 and k in _SMALL_GAUSSIAN:
        return np.array(_SMALL_GAUSSIAN[k], np.float64)
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    w = np.array([math.exp(-((i - k // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(k)], np.float64)
    return w / w.sum()


def gaussian_blur(img: torch.Tensor, ksize: Sequence[int], sigma: float = 0.0) -> torch.Tensor:
    """``cv2.GaussianBlur(img, ksize, sigma)`` for a float32 image (uint8 raises): ``ksize = (kw, kh)`` in cv2's order, both odd and ``<= 31``; each dimension
    of the image must exceed ``k // 2``.  ``sigma`` serves both axes.  Border ``BORDER_REFLECT_101``.  Both passes accumulate in double in a fixed order and
    the value is rounded to float once, which is nearer the real-number value than OpenCV's float coefficients and float sums."""
    H, W, C = _image("img", img, (torch.float32,))
    if not (isinstance(ksize, (tuple, list)) and len(ksize) == 2 and all(isinstance(x, (int, np.integer)) for x in ksize)):
        raise RuntimeError(f"ksize is a pair (kw, kh), got {ksize!r}")
    kw, kh = int(ksize[0]), int(ksize[1])
    if not (1 <= kw <= MAX_BLUR_KERNEL and 1 <= kh <= MAX_BLUR_KERNEL and kw % 2 and kh % 2):
        raise RuntimeError(f"ksize must be odd and at most {MAX_BLUR_KERNEL} in both dimensions, got ({kw}, {kh})")
    if H <= kh // 2 or W <= kw // 2:
        raise RuntimeError(f"each dimension of the image must exceed k // 2 (the reflected border): image {H}x{W}, ksize ({kw}, {kh})")
    dev = _need_device("mask_ops", img=img)
    src = img.detach()
    out = torch.empty(tuple(img.shape), dtype=torch.float32, device=dev)
    wx, wy = gaussian_kernel(kw, float(sigma)), gaussian_kernel(kh, float(sigma))
    ws, nbytes = _workspace(_lib.tgs_maskops_workspace_bytes(H, W, C, 8), dev)
    with _guard(dev):
        _ok(_lib.tgs_maskops_blur(_raw_stream(dev.index), H, W, C, src.data_ptr(), *_strides(src), kw, kh, wx.ctypes.data, wy.ctypes.data, out.data_ptr(), ws.data_ptr(), nbytes))
    return out
