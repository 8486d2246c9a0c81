"""The trainers' photometric loss on the MI355X ("next" row 2): drop-in for ``utils/loss_utils.py`` of the reference.

``l1_loss`` / ``l2_loss`` / ``ssim`` keep the reference's names and argument meaning (loss_utils.py:17-18, :20-21,
:33-63: the three names every trainer imports); ``l1_ssim_loss`` is the composition the trainers build for
``'l1+dssim'`` (tetgs_texture/refine.py:245-247).  Value and gradient of the SSIM losses come from two passes over the
image (csrc/tgs_loss.hip) instead of five depthwise convolutions, ~15 element-wise kernels and their autograd graph;
``l2_loss`` and ``pixel_value_and_grad`` are one pointwise pass each way.  ``l1_ssim_value_and_grad`` and
``pixel_value_and_grad`` are the forms without autograd for ``multiview.SyncFreeBatch``.  HIP device only: there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch

from .diff_gaussian_rasterization import _C as _rast_c

_lib = _rast_c._lib
_lib.tgs_l1_ssim_workspace_bytes.restype = C.c_size_t
_lib.tgs_l1_ssim_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
_lib.tgs_l1_ssim.restype = C.c_int
_lib.tgs_l1_ssim.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]


def _check(img: torch.Tensor, gt: torch.Tensor) -> Tuple[int, int, int]:
    if not img.is_cuda or not gt.is_cuda:
        raise RuntimeError("youreditableavatar_amd.loss has no CPU path: images must be on a HIP device")
    if img.shape != gt.shape or img.dim() not in (3, 4):
        raise RuntimeError(f"expected two images of the same [C,H,W] or [B,C,H,W] shape, got {tuple(img.shape)} and {tuple(gt.shape)}")
    if img.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("expected float32 images")
    planes = int(img.shape[0]) if img.dim() == 3 else int(img.shape[0] * img.shape[1])
    return planes, int(img.shape[-2]), int(img.shape[-1])


def _images(img: torch.Tensor) -> Tuple[int, int]:
    """(images, channels) of a checked [C,H,W] (one image) or [B,C,H,W] tensor"""
    return (1, int(img.shape[0])) if img.dim() == 3 else (int(img.shape[0]), int(img.shape[1]))


def l1_ssim_value_and_grad(img: torch.Tensor, gt: torch.Tensor, dssim_factor: float = 0.2, need_grad: bool = True, per_image: bool = False):
    """-> (out3, grad): out3 = device tensor [loss, ssim, l1]; grad = d loss / d img (None unless ``need_grad``).
    Nothing is synchronised; use this directly as the ``upstream`` of ``multiview.SyncFreeBatch``.

    ``per_image=True``: out3 is ``[B,3]``, one (loss, ssim, l1) per image of the ``[B,C,H,W]`` batch (``[C,H,W]``: B = 1), and
    grad is the gradient of the SUM of the per-image losses -- divide by the number of views for their mean."""
    planes, H, W = _check(img, gt)
    dev = img.device
    a, b = img.detach().contiguous(), gt.detach().contiguous()
    if per_image:
        B, Cn = _images(img)
        with torch.cuda.device(dev):
            nbytes = int(_lib.tgs_l1_ssim_images_workspace_bytes(B, Cn, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(B, 3, dtype=torch.float32, device=dev)
            grad = torch.empty_like(a) if need_grad else None
            r = _lib.tgs_l1_ssim_images(torch.cuda.current_stream(dev).cuda_stream, B, Cn, H, W, a.data_ptr(), b.data_ptr(), float(dssim_factor),
                                        out.data_ptr(), grad.data_ptr() if need_grad else None, ws.data_ptr(), nbytes)
        if r < 0:
            raise _rast_c._err(r)
        return out, grad
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_l1_ssim_workspace_bytes(planes, H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        grad = torch.empty_like(a) if need_grad else None
        r = _lib.tgs_l1_ssim(torch.cuda.current_stream(dev).cuda_stream, planes, H, W, a.data_ptr(), b.data_ptr(), float(dssim_factor),
                             out3.data_ptr(), grad.data_ptr() if need_grad else None, ws.data_ptr(), nbytes)
    if r < 0:
        raise _rast_c._err(r)
    return out3, grad


_lib.tgs_l1_ssim_backward.restype = C.c_int
_lib.tgs_l1_ssim_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]


class _L1SSIM(torch.autograd.Function):
    """Forward: the statistics pass + the reduction (value only); the gradient pass runs in backward with the incoming gradient as a device
    scalar folded in (tgs_l1_ssim_backward) -- no image-sized ``grad * g`` pass, and no gradient image is computed for a loss that is never
    back-propagated."""

    @staticmethod
    def forward(ctx, img, gt, dssim_factor, which):
        planes, H, W = _check(img, gt)
        dev = img.device
        a, b = img.detach().contiguous(), gt.detach().contiguous()
        with torch.cuda.device(dev):
            nbytes = int(_lib.tgs_l1_ssim_workspace_bytes(planes, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out3 = torch.empty(3, dtype=torch.float32, device=dev)
            r = _lib.tgs_l1_ssim(torch.cuda.current_stream(dev).cuda_stream, planes, H, W, a.data_ptr(), b.data_ptr(), float(dssim_factor),
                                 out3.data_ptr(), None, ws.data_ptr(), nbytes)
        if r < 0:
            raise _rast_c._err(r)
        ctx.save_for_backward(a, b, ws)
        ctx.dims, ctx.f, ctx.shape = (planes, H, W), float(dssim_factor), img.shape
        return out3[which]

    @staticmethod
    def backward(ctx, g):
        a, b, ws = ctx.saved_tensors
        planes, H, W = ctx.dims
        dev = a.device
        g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(a)
        with torch.cuda.device(dev):
            r = _lib.tgs_l1_ssim_backward(torch.cuda.current_stream(dev).cuda_stream, planes, H, W, a.data_ptr(), b.data_ptr(), ctx.f, g.data_ptr(),
                                          grad.data_ptr(), ws.data_ptr(), ws.numel())
        if r < 0:
            raise _rast_c._err(r)
        return grad.view(ctx.shape), None, None, None


def l1_ssim_loss(network_output: torch.Tensor, gt: torch.Tensor, dssim_factor: float = 0.2) -> torch.Tensor:
    """``(1 - dssim_factor) * l1_loss(x, gt) + dssim_factor * (1 - ssim(x, gt))`` (refine.py:245-247), differentiable in x."""
    return _L1SSIM.apply(network_output, gt, float(dssim_factor), 0)


_lib.tgs_l1_ssim_images_workspace_bytes.restype = C.c_size_t
_lib.tgs_l1_ssim_images_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
_lib.tgs_l1_ssim_images.restype = C.c_int
_lib.tgs_l1_ssim_images.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_l1_ssim_images_backward.restype = C.c_int
_lib.tgs_l1_ssim_images_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_size_t]


class _L1SSIMImages(torch.autograd.Function):
    """_L1SSIM with one value per image: forward returns column ``which`` of out[B,3]; backward hands the incoming [B] gradient to the
    gradient pass as it is (tgs_l1_ssim_images_backward picks image blockIdx.z / channels' entry)."""

    @staticmethod
    def forward(ctx, img, gt, dssim_factor, which):
        _planes, H, W = _check(img, gt)
        B, Cn = _images(img)
        dev = img.device
        a, b = img.detach().contiguous(), gt.detach().contiguous()
        with torch.cuda.device(dev):
            nbytes = int(_lib.tgs_l1_ssim_images_workspace_bytes(B, Cn, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(B, 3, dtype=torch.float32, device=dev)
            r = _lib.tgs_l1_ssim_images(torch.cuda.current_stream(dev).cuda_stream, B, Cn, H, W, a.data_ptr(), b.data_ptr(), float(dssim_factor),
                                        out.data_ptr(), None, ws.data_ptr(), nbytes)
        if r < 0:
            raise _rast_c._err(r)
        ctx.save_for_backward(a, b, ws)
        ctx.dims, ctx.f, ctx.shape = (B, Cn, H, W), float(dssim_factor), img.shape
        return out[:, which]

    @staticmethod
    def backward(ctx, g):
        a, b, ws = ctx.saved_tensors
        B, Cn, H, W = ctx.dims
        dev = a.device
        g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(a)
        with torch.cuda.device(dev):
            r = _lib.tgs_l1_ssim_images_backward(torch.cuda.current_stream(dev).cuda_stream, B, Cn, H, W, a.data_ptr(), b.data_ptr(), ctx.f, g.data_ptr(), 1,
                                                 grad.data_ptr(), ws.data_ptr(), ws.numel())
        if r < 0:
            raise _rast_c._err(r)
        return grad.view(ctx.shape), None, None, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """loss_utils.py:33-63 with window 11, differentiable in ``img1``: the mean over everything, or with ``size_average=False`` one
    value per image of a ``[B,C,H,W]`` batch (a ``[B]`` tensor)."""
    if window_size != 11:
        raise NotImplementedError("the fused kernel implements the window the reference uses: window_size=11")
    if size_average:
        return 1.0 - _L1SSIM.apply(img1, img2, 1.0, 0)
    if img1.dim() != 4:
        # the reference's ssim_map.mean(1).mean(1).mean(1) (loss_utils.py:63) runs out of dimensions on a [C,H,W] map
        raise IndexError("ssim(size_average=False) returns one value per image and needs a [B,C,H,W] batch: "
                         f"got {img1.dim()} dimensions (the reference's mean(1).mean(1).mean(1) fails the same way)")
    return 1.0 - _L1SSIMImages.apply(img1, img2, 1.0, 0)


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """loss_utils.py:17-18."""
    return _L1SSIM.apply(network_output, gt, 0.0, 0)


_KINDS = {"l1": 0, "l2": 1}                     # TGS_LOSS_L1, TGS_LOSS_L2
_lib.tgs_pixel_loss_workspace_bytes.restype = C.c_size_t
_lib.tgs_pixel_loss_workspace_bytes.argtypes = [C.c_int, C.c_int64]
_lib.tgs_pixel_loss.restype = C.c_int
_lib.tgs_pixel_loss.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_pixel_loss_backward.restype = C.c_int
_lib.tgs_pixel_loss_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


def _check_pixel(img: torch.Tensor, gt: torch.Tensor) -> None:
    if not img.is_cuda or not gt.is_cuda:
        raise RuntimeError("youreditableavatar_amd.loss has no CPU path: tensors must be on a HIP device")
    if img.shape != gt.shape or img.numel() == 0:
        raise RuntimeError(f"expected two non-empty tensors of the same shape, got {tuple(img.shape)} and {tuple(gt.shape)}")
    if img.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("expected float32 tensors")


def _pixel_forward(kind: int, a: torch.Tensor, b: torch.Tensor, images: int, need_grad: bool):
    dev = a.device
    n = a.numel() // images
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_pixel_loss_workspace_bytes(images, n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(images, dtype=torch.float32, device=dev)
        grad = torch.empty_like(a) if need_grad else None
        r = _lib.tgs_pixel_loss(torch.cuda.current_stream(dev).cuda_stream, kind, images, n, a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                grad.data_ptr() if need_grad else None, ws.data_ptr(), nbytes)
    if r < 0:
        raise _rast_c._err(r)
    return out, grad


def pixel_value_and_grad(img: torch.Tensor, gt: torch.Tensor, kind: str = "l2", per_image: bool = False, need_grad: bool = True):
    """The pointwise loss of the trainers' ``'l1'`` / ``'l2'`` settings without autograd, for ``multiview.SyncFreeBatch``:
    -> (value, grad) with value a device scalar (``per_image=True``: ``[B]``, one mean per image of the batch's first dimension, and
    grad the gradient of their SUM) and grad = d value / d img (None unless ``need_grad``).  One pass over the two tensors; nothing is
    synchronised, nothing is recorded for autograd."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be 'l1' or 'l2', got {kind!r}")
    _check_pixel(img, gt)
    if per_image and img.dim() < 2:
        raise RuntimeError("per_image=True needs a batch dimension in front of the image's")
    a, b = img.detach().contiguous(), gt.detach().contiguous()
    out, grad = _pixel_forward(_KINDS[kind], a, b, int(img.shape[0]) if per_image else 1, need_grad)
    return (out if per_image else out[0]), grad


class _PixelLoss(torch.autograd.Function):
    """Forward: the value pass (two reads per element); backward: the gradient pass (two reads, one write) with the incoming gradient as
    a device scalar folded in (tgs_pixel_loss_backward)."""

    @staticmethod
    def forward(ctx, img, gt, kind):
        _check_pixel(img, gt)
        a, b = img.detach().contiguous(), gt.detach().contiguous()
        out, _ = _pixel_forward(kind, a, b, 1, False)
        ctx.save_for_backward(a, b)
        ctx.kind, ctx.shape = kind, img.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        dev = a.device
        g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(a)
        with torch.cuda.device(dev):
            r = _lib.tgs_pixel_loss_backward(torch.cuda.current_stream(dev).cuda_stream, ctx.kind, 1, a.numel(), a.data_ptr(), b.data_ptr(), g.data_ptr(), 0,
                                             grad.data_ptr())
        if r < 0:
            raise _rast_c._err(r)
        return grad.view(ctx.shape), None, None


def l2_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """loss_utils.py:20-21: ``((network_output - gt) ** 2).mean()``, differentiable in ``network_output``."""
    return _PixelLoss.apply(network_output, gt, _KINDS["l2"])
