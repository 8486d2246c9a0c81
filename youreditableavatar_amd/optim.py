"""The trainers' optimizer step on the MI355X: drop-in for ``torch.optim.Adam`` as ``Edit_core/tetgs_scene/tetgs_optimizer.py`` builds it.

The reference runs ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` over up to six parameter groups (tetgs_optimizer.py:92, :167) and steps it
once per iteration (:101-103, :176-178); on a HIP device that is torch's foreach path, about seven multi-tensor element-wise kernels that
each stream every parameter-sized tensor again.  ``FusedAdam.step()`` is ONE launch of ``tgs_adam_step`` (csrc/tgs_optim.hip) for all
tensors of all groups: 4 reads and 3 writes per parameter float.  It reads the level-major ``.grad`` that
``multiview.FlatGradients(level_major=True)`` gives the SH parameters as it is, and folds a ``grad_scale`` (1 / views for the mean of a
batch's per-image losses) into the gradient load.  ``GaussianOptimizer`` is the wrapper the trainers call (``TetGSOptimizer`` /
``EditTetGSOptimizer``), ``expon_lr`` its position schedule.  HIP device only: there is no CPU fallback; construction needs no device.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Mapping, Optional, Tuple

import torch

from .diff_gaussian_rasterization import _C as _rast_c

_lib = _rast_c._lib


class _AdamTensor(C.Structure):             # tgs_adam_tensor_t
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64),
                ("grad_plane_stride", C.c_int64), ("planes", C.c_int32), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("reserved", C.c_int32)]


_lib.tgs_sizeof_adam_tensor.restype = C.c_size_t
_lib.tgs_sizeof_adam_tensor.argtypes = []
if _lib.tgs_sizeof_adam_tensor() != C.sizeof(_AdamTensor):
    raise ImportError(f"libtgs_raster.so was built with another tgs_adam_tensor_t ({_lib.tgs_sizeof_adam_tensor()} bytes, this binding: {C.sizeof(_AdamTensor)})")
_lib.tgs_adam_max_tensors.restype = C.c_int
_lib.tgs_adam_max_tensors.argtypes = []
MAX_TENSORS_PER_LAUNCH = int(_lib.tgs_adam_max_tensors())     # a step with more tensors becomes several launches (inside tgs_adam_step)
_lib.tgs_adam_step.restype = C.c_int
_lib.tgs_adam_step.argtypes = [C.c_void_p, C.POINTER(_AdamTensor), C.c_int, C.c_double, C.c_double, C.c_float, C.c_float]

MAX_PLANES = 64                             # level-major gradients: M of the [P, M, 3] parameter (csrc/tgs_optim.hip: ADAM_MAX_PLANES)


def grad_layout(p: torch.Tensor, grad: torch.Tensor) -> Tuple[int, int]:
    """-> (plane stride in floats, planes) of a gradient the kernel reads in place: (0, 0) for a contiguous one, (stride, M) for the
    level-major view ``FlatGradients(level_major=True)`` makes of a ``[P, M, 3]`` parameter -- element (p, m, c) at
    ``m * stride + 3 p + c``.  Anything else is refused: it is not silently copied."""
    if grad.is_sparse:
        raise RuntimeError("FusedAdam does not support sparse gradients")
    if grad.shape != p.shape or grad.dtype != torch.float32 or grad.device != p.device:
        raise RuntimeError(f"FusedAdam: .grad must be a float32 tensor of the parameter's shape on its device, got {tuple(grad.shape)} {grad.dtype} on {grad.device}")
    if grad.is_contiguous():
        return 0, 0
    st = grad.stride()
    if (p.dim() == 3 and int(p.shape[2]) == 3 and 1 <= int(p.shape[1]) <= MAX_PLANES and st[0] == 3 and st[2] == 1 and st[1] >= 3 * int(p.shape[0]) and st[1] % 4 == 0
            and grad.data_ptr() % 16 == 0):
        return int(st[1]), int(p.shape[1])
    raise RuntimeError("FusedAdam: .grad must be contiguous, or the level-major view FlatGradients(level_major=True) makes of a [P, M, 3] parameter "
                       f"(strides (3, plane, 1), plane >= 3 P a multiple of 4, 16-byte aligned, M <= {MAX_PLANES}); got shape {tuple(grad.shape)} with strides {tuple(st)}")


def _check_tensor(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"FusedAdam: {what} must be a contiguous float32 tensor, got {t.dtype} with strides {tuple(t.stride())}")


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` for fp32 parameters on a HIP device, one kernel launch per ``step()``.

    Same constructor arguments, the same per-parameter state (``step``: a host scalar tensor, ``exp_avg``, ``exp_avg_sq``) and the same
    group keys as ``torch.optim.Adam``: a ``state_dict`` saved by either loads into the other.  Torch's semantics are kept: a parameter
    whose ``.grad`` is ``None`` is skipped (no state, no step count), ``lr`` is read from its group at every step (0 is legal), the step
    count is per parameter.  ``weight_decay``, ``amsgrad``, ``maximize``, ``capturable`` and ``differentiable`` raise
    ``NotImplementedError``.  ``step(grad_scale=s)`` is Adam on ``grad * s``, the product formed at the gradient load."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0, amsgrad: bool = False, *,
                 foreach: Optional[bool] = None, maximize: bool = False, capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 decoupled_weight_decay: bool = False):
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("FusedAdam takes lr and betas as Python floats (they are host scalars of the launch)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        # torch.optim.Adam's keys, so that param_groups travel between the two through state_dict (foreach / fused are torch's choice of
        # implementation and mean nothing here)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach, capturable=capturable,
                        differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        self._check_group(defaults)
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group) -> None:
        if group.get("weight_decay", 0) != 0:
            raise NotImplementedError("FusedAdam: weight_decay != 0 is not implemented (the reference's trainers use none)")
        for key in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(key, False):
                raise NotImplementedError(f"FusedAdam: {key}=True is not implemented")

    def _init_state(self, p: torch.Tensor) -> dict:
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)     # torch's host scalar
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif state["step"].device.type != "cpu":             # a state_dict of torch.optim.Adam(fused=True / capturable=True): the count moves to the host once
            state["step"] = state["step"].detach().to("cpu")
        return state

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None, grad_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # launches: tensors of one device with one (beta1, beta2, eps) -- for the trainers' optimizer that is ONE for all groups
        launches: Dict[tuple, List[tuple]] = {}
        for group in self.param_groups:
            self._check_group(group)
            lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
            if isinstance(lr, torch.Tensor) or isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor):
                raise NotImplementedError("FusedAdam takes lr and betas as Python floats")
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check_tensor(p, "a parameter")
                plane, planes = grad_layout(p, p.grad)
                if not p.is_cuda:
                    raise RuntimeError("youreditableavatar_amd.optim has no CPU path: parameters must be on a HIP device")
                state = self._init_state(p)
                for key in ("exp_avg", "exp_avg_sq"):
                    _check_tensor(state[key], key)
                    if state[key].shape != p.shape or state[key].device != p.device:
                        raise RuntimeError(f"FusedAdam: {key} must have the parameter's shape and device")
                state["step"] += 1
                t = int(state["step"].item())
                step_size = float(lr) / (1 - beta1 ** t)
                bc2_sqrt = (1 - beta2 ** t) ** 0.5
                launches.setdefault((p.device, float(beta1), float(beta2), float(eps)), []).append((p, state, plane, planes, step_size, bc2_sqrt))
        for (dev, beta1, beta2, eps), items in launches.items():
            table = (_AdamTensor * len(items))()
            for e, (p, state, plane, planes, step_size, bc2_sqrt) in zip(table, items):
                e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()
                e.numel, e.grad_plane_stride, e.planes, e.step_size, e.bc2_sqrt = p.numel(), plane, planes, step_size, bc2_sqrt
            with torch.cuda.device(dev):
                r = _lib.tgs_adam_step(torch.cuda.current_stream(dev).cuda_stream, table, len(items), beta1, beta2, eps, float(grad_scale))
            if r < 0:
                raise _rast_c._err(r)
        return loss


def expon_lr(lr_init: float, lr_final: float, lr_delay_steps: int = 0, lr_delay_mult: float = 1.0, max_steps: int = 1_000_000) -> Callable[[float], float]:
    """The position schedule of the trainers (``get_expon_lr_func``, Edit_core/utils/general_utils.py:25-58): log-linear interpolation from
    ``lr_init`` at step 0 to ``lr_final`` at ``max_steps`` (held beyond), times -- with ``lr_delay_steps > 0`` -- a sine ramp from
    ``lr_delay_mult`` to 1 over the first ``lr_delay_steps``; 0 for a negative step or when both rates are 0."""
    def lr(step: float) -> float:
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        t = min(max(step / max_steps, 0.0), 1.0)
        rate = math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
        if lr_delay_steps > 0:
            rate *= lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        return rate
    return lr


@dataclass
class OptimizationParams:
    """The reference's record of the same name (tetgs_optimizer.py:9-31): its field names and defaults."""
    iterations: int = 15_000
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30_000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001


class GaussianOptimizer:
    """What the trainers call on ``TetGSOptimizer`` / ``EditTetGSOptimizer`` (tetgs_optimizer.py:47-125, :128-200), over ``FusedAdam``.

    ``params``: group name -> tensor, any of ``"points"``, ``"sh_coordinates_dc"``, ``"sh_coordinates_rest"``, ``"all_densities"``,
    ``"scales"``, ``"quaternions"``; a name that is absent is not optimised (the reference's ``learn_*`` / ``freeze_gaussians`` flags).  The
    groups are built in the reference's order with its learning rates: ``"points"`` starts at ``position_lr_init * spatial_lr_scale`` and
    follows ``expon_lr`` through ``update_learning_rate``; ``"sh_coordinates_rest"`` gets ``feature_lr / 20``."""

    GROUPS = ("points", "sh_coordinates_dc", "sh_coordinates_rest", "all_densities", "scales", "quaternions")

    def __init__(self, params: Mapping[str, torch.Tensor], opt: Optional[OptimizationParams] = None, spatial_lr_scale: float = 1.0):
        if opt is None:
            opt = OptimizationParams()
        unknown = sorted(set(params) - set(self.GROUPS))
        if unknown:
            raise ValueError(f"unknown parameter groups {unknown}: expected names out of {self.GROUPS}")
        self.current_iteration = 0
        self.num_iterations = opt.iterations
        self.spatial_lr_scale = spatial_lr_scale
        rates = {"points": opt.position_lr_init * spatial_lr_scale, "sh_coordinates_dc": opt.feature_lr, "sh_coordinates_rest": opt.feature_lr / 20.0,
                 "all_densities": opt.opacity_lr, "scales": opt.scaling_lr, "quaternions": opt.rotation_lr}
        groups = [{"params": [params[name]], "lr": rates[name], "name": name} for name in self.GROUPS if name in params]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        self.position_sheduler_func = expon_lr(lr_init=opt.position_lr_init * spatial_lr_scale, lr_final=opt.position_lr_final * spatial_lr_scale,
                                               lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)      # (the reference's spelling)

    def step(self, grad_scale: float = 1.0) -> None:
        self.optimizer.step(grad_scale=grad_scale)
        self.current_iteration += 1

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def update_learning_rate(self, iteration: Optional[int] = None) -> float:
        if iteration is None:
            iteration = self.current_iteration
        lr = 0.0
        for group in self.optimizer.param_groups:
            if group["name"] == "points":
                lr = self.position_sheduler_func(iteration)
                group["lr"] = lr
        return lr

    def add_param_group(self, new_param_group: dict) -> None:
        self.optimizer.add_param_group(new_param_group)

    def state_dict(self) -> dict:
        return self.optimizer.state_dict()

    def load_state_dict(self, state_dict: dict) -> None:
        self.optimizer.load_state_dict(state_dict)
