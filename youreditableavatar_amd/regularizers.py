"""The scaling regulariser of the reference's refinement loops, fused and without a host synchronisation.

Every iteration of ``tetgs_texture/refine.py:306-317`` and ``refine_3dgs.py:339-350`` (``scaling_reg = True`` is the default, refine.py:42) runs

    radii = tetgs.radii                                     # tetgs_model.py:299-310 / tetgs_edit_3d.py:332-343: rebuilt from the mesh each time
    max_vals, _ = torch.max(tetgs.scaling, dim=-1);  min_vals, _ = torch.min(tetgs.scaling, dim=-1)
    thresh_idxs = (max_vals > radii * 1.0) & (max_vals / min_vals > 10.0)
    if thresh_idxs.sum() > 0:                               # a host read-back per step
        loss = loss + max_vals[thresh_idxs].mean() * 1.0

``gaussian_radii`` computes the radii once (the mesh vertices are fixed buffers); ``scaling_regularizer`` (on the activated scales) and
``scaling_regularizer_raw`` (on the raw ``_scales``, the ``exp`` inside the kernel) return the term as a 0-dim tensor that is **0 with a zero
gradient when no row is selected** -- what the reference's ``if`` amounts to -- so nothing is read back; ``scaling_reg_value_and_grad`` is
the form without autograd for ``multiview.SyncFreeBatch``-style steps.  On tied maxima the gradient goes to the lowest index, as
``torch.max(dim=-1)`` does on the CPU.  Kernels: csrc/tgs_reg.hip (C ABI tgs_gaussian_radii / tgs_scale_reg_forward / _backward).  HIP tensors
only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .diff_gaussian_rasterization import _C as _rast_c

_lib = _rast_c._lib
_lib.tgs_gaussian_radii.restype = C.c_int
_lib.tgs_gaussian_radii.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
_lib.tgs_scale_reg_workspace_bytes.restype = C.c_size_t
_lib.tgs_scale_reg_workspace_bytes.argtypes = [C.c_int]
_lib.tgs_scale_reg_forward.restype = C.c_int
_lib.tgs_scale_reg_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.tgs_scale_reg_backward.restype = C.c_int
_lib.tgs_scale_reg_backward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]

_INDEX_KINDS = {torch.int32: 0, torch.int64: 1, torch.float32: 2}        # TGS_INDEX_I32 / _I64 / _F32


def _on_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"regularizers (MI355X build) has no CPU path: {name} must be on a HIP device")


def gaussian_radii(verts: torch.Tensor, faces: torch.Tensor, face_indices: torch.Tensor) -> torch.Tensor:
    """The ``radii`` property of ``TetGS`` / ``Edit3DTetGS`` (tetgs_model.py:299-310, tetgs_edit_3d.py:332-343): the circumradius
    ``a b c / (4 sqrt(s (s-a) (s-b) (s-c)))`` (utils/graphics_utils.py:109-116) of every Gaussian's face, ``[P]`` float32, in one kernel
    (evaluated in double).  ``verts [V,3]`` float32, ``faces [F,3]`` int32 / int64, ``face_indices [P]`` or ``[P,1]`` of an integer or
    floating dtype (floats are truncated as ``.int()`` does, tetgs_edit_3d.py:341).  A degenerate face gives ``inf`` or NaN as the
    reference's formula does; an index out of range raises.  Meant to run ONCE per model: it reads one flag back."""
    for name, t in (("verts", verts), ("faces", faces), ("face_indices", face_indices)):
        _on_device(t, name)
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"verts must be [V,3] float32, got {tuple(verts.shape)} {verts.dtype}")
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"faces must be [F,3] int32 or int64, got {tuple(faces.shape)} {faces.dtype}")
    if face_indices.dim() > 2 or (face_indices.dim() == 2 and face_indices.shape[1] != 1) or face_indices.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise RuntimeError(f"face_indices must be [P] or [P,1] of an integer or floating dtype, got {tuple(face_indices.shape)} {face_indices.dtype}")
    dev = verts.device
    idx = face_indices.detach().reshape(-1)
    if idx.dtype not in _INDEX_KINDS:
        idx = idx.to(torch.int64)                          # truncation toward zero, like .int()
    v, f, idx = verts.detach().contiguous(), faces.to(dev).contiguous(), idx.to(dev).contiguous()
    P = int(idx.shape[0])
    with torch.cuda.device(dev):
        radii = torch.empty(P, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        r = _lib.tgs_gaussian_radii(torch.cuda.current_stream(dev).cuda_stream, int(v.shape[0]), int(f.shape[0]), P, v.data_ptr(), f.data_ptr(),
                                    int(f.dtype == torch.int64), idx.data_ptr(), _INDEX_KINDS[idx.dtype], radii.data_ptr(), flag.data_ptr())
    if r < 0:
        raise _rast_c._err(r)
    if P and int(flag.item()):
        raise RuntimeError(f"gaussian_radii: a face index outside [0, {int(f.shape[0])}) or a vertex index outside [0, {int(v.shape[0])}) (TGS_ERR_INVALID)")
    return radii


def _check(scales: torch.Tensor, radii: torch.Tensor, name: str) -> int:
    _on_device(scales, name)
    _on_device(radii, "radii")
    if scales.dtype != torch.float32 or radii.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float but found {scales.dtype} for {name} and {radii.dtype} for radii")
    if scales.dim() != 2 or scales.shape[1] != 3:
        raise RuntimeError(f"{name} must be [P,3], got {tuple(scales.shape)}")
    if radii.numel() != scales.shape[0]:
        raise RuntimeError(f"radii must have one value per Gaussian ({int(scales.shape[0])} Gaussians), got {tuple(radii.shape)}")
    return int(scales.shape[0])


def _forward(s: torch.Tensor, r: torch.Tensor, raw: bool, max_factor: float, ratio_threshold: float):
    """-> (codes [P] uint8, out3: float32[3] holding value, the count's bits, 1 / count); ``s`` / ``r`` contiguous, on one device"""
    dev, P = s.device, int(s.shape[0])
    with torch.cuda.device(dev):
        nbytes = int(_lib.tgs_scale_reg_workspace_bytes(P))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        codes = torch.empty(P, dtype=torch.uint8, device=dev)
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        rc = _lib.tgs_scale_reg_forward(torch.cuda.current_stream(dev).cuda_stream, P, s.data_ptr() if P else None, int(raw), r.data_ptr() if P else None,
                                        float(max_factor), float(ratio_threshold), codes.data_ptr() if P else None, out3.data_ptr(), ws.data_ptr() if P else None, nbytes)
    if rc < 0:
        raise _rast_c._err(rc)
    return codes, out3


def _backward(codes: torch.Tensor, out3: torch.Tensor, raw_scales: Optional[torch.Tensor], upstream: Optional[torch.Tensor], weight: float, accumulate: bool,
              grad: torch.Tensor) -> None:
    dev, P = grad.device, int(codes.shape[0])
    if P == 0:
        return
    with torch.cuda.device(dev):
        rc = _lib.tgs_scale_reg_backward(torch.cuda.current_stream(dev).cuda_stream, P, codes.data_ptr(), out3.data_ptr(), None if raw_scales is None else raw_scales.data_ptr(),
                                         None if upstream is None else upstream.data_ptr(), float(weight), int(accumulate), grad.data_ptr())
    if rc < 0:
        raise _rast_c._err(rc)


class _ScaleReg(torch.autograd.Function):
    """Forward: the decision pass + the reduction; backward: one pass that reads the forward's code bytes (the rows are never decided twice)
    with the incoming gradient as a device scalar folded in."""

    @staticmethod
    def forward(ctx, scales, radii, max_factor, ratio_threshold, raw):
        P = _check(scales, radii, "raw_scales" if raw else "scaling")
        dev = scales.device
        s, r = scales.detach().contiguous(), radii.detach().reshape(-1).to(dev).contiguous()
        codes, out3 = _forward(s, r, raw, max_factor, ratio_threshold)
        ctx.save_for_backward(codes, out3, s if raw else torch.Tensor([]))
        ctx.P, ctx.raw = P, raw
        ctx.mark_non_differentiable(codes)
        return out3[0], codes

    @staticmethod
    def backward(ctx, g, _g_codes):
        codes, out3, s = ctx.saved_tensors
        dev = codes.device
        g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty((ctx.P, 3), dtype=torch.float32, device=dev)
        _backward(codes, out3, s if ctx.raw else None, g, 1.0, False, grad)
        return grad, None, None, None, None


def scaling_regularizer(scaling: torch.Tensor, radii: torch.Tensor, max_factor: float = 1.0, ratio_threshold: float = 10.0, return_codes: bool = False):
    """The loop's term (module docstring) on the ACTIVATED scales ``[P,3]`` -- ``tetgs.scaling``, or a contiguous row slice of
    ``gaussian_bind_groups``' output for ``edit_scaling`` -- and ``radii [P]`` (``gaussian_radii``): the mean of ``max`` over the rows with
    ``max > radii * max_factor`` and ``max / min > ratio_threshold``, a 0-dim tensor, differentiable in ``scaling``; 0 with a zero gradient
    when no row qualifies.  ``return_codes=True``: also the per-row code bytes (0 = not selected, 1..3 = index of the maximum + 1)."""
    value, codes = _ScaleReg.apply(scaling, radii, float(max_factor), float(ratio_threshold), False)
    return (value, codes) if return_codes else value


def scaling_regularizer_raw(raw_scales: torch.Tensor, radii: torch.Tensor, max_factor: float = 1.0, ratio_threshold: float = 10.0, return_codes: bool = False):
    """``scaling_regularizer(torch.exp(raw_scales), radii, ...)`` without the ``scaling`` tensor: the activation is applied inside the
    kernels (the same ``expf`` as ``gaussian_bind``), and the gradient arrives at the raw ``_scales`` directly."""
    value, codes = _ScaleReg.apply(raw_scales, radii, float(max_factor), float(ratio_threshold), True)
    return (value, codes) if return_codes else value


def scaling_reg_value_and_grad(raw_scales: torch.Tensor, radii: torch.Tensor, max_factor: float = 1.0, ratio_threshold: float = 10.0,
                               grad_out: Optional[torch.Tensor] = None, accumulate: bool = False, weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The raw form without autograd -> (value, grad): value a device scalar (the unweighted term), grad ``[P,3]`` the gradient of
    ``weight * value`` with respect to ``raw_scales`` -- written to ``grad_out`` (every element; a new tensor when it is None), or with
    ``accumulate=True`` ADDED to ``grad_out``, the step's gradient buffer of ``_scales``.  Nothing is synchronised."""
    P = _check(raw_scales, radii, "raw_scales")
    dev = raw_scales.device
    s, r = raw_scales.detach().contiguous(), radii.detach().reshape(-1).to(dev).contiguous()
    if grad_out is None:
        if accumulate:
            raise RuntimeError("scaling_reg_value_and_grad: accumulate=True needs the gradient buffer to add to (grad_out)")
        grad_out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    else:
        _on_device(grad_out, "grad_out")
        if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (P, 3) or not grad_out.is_contiguous() or grad_out.device != dev:
            raise RuntimeError(f"grad_out must be a contiguous [{P},3] float32 tensor on {dev}, got {tuple(grad_out.shape)} {grad_out.dtype}")
    codes, out3 = _forward(s, r, True, max_factor, ratio_threshold)
    _backward(codes, out3, s, None, weight, accumulate, grad_out)
    return out3[0], grad_out
