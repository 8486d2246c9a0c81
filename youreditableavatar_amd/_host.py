"""The host layer under the geometry stage's modules (private): ``_mesh`` (and through it ``mesh_raster``, ``mesh_raster_aa``, ``mesh_raster_grad``),
``marching_tets``, ``mesh_geom``, ``hashgrid`` and ``tet_grid``.

Written once here: the ctypes aliases of the signature tables and ``declare``, which applies one; the handle of the native library; ``ok``, which raises
the library's error; the device guard that is entered only when the device is not the current one, and the raw stream number; the device check that
comes last in every argument check; and the small conversions every call makes: a tensor's address or NULL, a workspace of so many bytes, an index array
as rows the kernels can load whole, and the error for an index outside the mesh or the grid.  Each module keeps its own ``SIGNATURES`` table, its
``declare(lib)`` and its ``_lib``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch

from .diff_gaussian_rasterization import _C as _rast_c

_P, _I, _L, _Z, _F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
lib = _rast_c._lib                                                              # once: every module declares its entry points on this handle


def declare(lib: C.CDLL, signatures: dict) -> C.CDLL:
    """applies a table ``name: (restype, argtypes)`` to a handle of the native library -> the handle"""
    for name, (restype, argtypes) in signatures.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    return lib


def ok(r: int) -> None:
    if r < 0:
        raise _rast_c._err(r)


NO_GUARD = contextlib.nullcontext()


def guard(dev: torch.device):
    """the device guard of a native call: entered only when ``dev`` is not the current device (the guard costs more than the test)"""
    return torch.cuda.device(dev) if torch.cuda.current_device() != dev.index else NO_GUARD


# torch.cuda.current_stream(dev).cuda_stream builds a Stream object per call (1.9 us of a 17 us call); torch has the number itself, under a private name
raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
    lambda index: torch.cuda.current_stream(index).cuda_stream)                # (the public way, should the private name go)


def need_device(module_name: str, **tensors) -> torch.device:
    """checked last, behind everything that can be said about the arguments without a device -> the one device"""
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"youreditableavatar_amd.{module_name} has no CPU path: {name} must be on a HIP device")
    devs = {t.device for t in tensors.values()}
    if len(devs) != 1:
        raise RuntimeError("all tensors must be on one device, got " + ", ".join(f"{n} on {t.device}" for n, t in tensors.items()))
    return next(iter(devs))


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def workspace(nbytes: int, dev: torch.device):
    """what a ``*_workspace_bytes`` function returned -> (the uint8 tensor of that size, the size)"""
    nbytes = int(nbytes)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def index_rows(t: torch.Tensor) -> torch.Tensor:
    """an index array [F,4] as the kernels load it: contiguous, and not starting inside a row's 16 bytes (such a view is copied)"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def index_error(name: str, n: int, owner: str) -> RuntimeError:
    """the error behind a read-back whose index flag is set; ``owner``: what has the ``n`` rows"""
    return RuntimeError(f"{name} holds a vertex index outside [0, {n}): {owner} (code -1)")
