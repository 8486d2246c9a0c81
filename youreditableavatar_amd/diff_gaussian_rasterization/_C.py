"""``_C`` -- the native-extension surface of the reference package.

The three pybind11 exports of the reference (diff-gaussian-rasterization/ext.cpp:15-19, signatures
rasterize_points.h:18-67) -- ``rasterize_gaussians``, ``rasterize_gaussians_backward``, ``mark_visible`` -- are served by the COMPILED
module ``_Cext`` (csrc/tgs_torch_ext.cpp: pybind11 + torch::Tensor glue over the C ABI of include/tgs_raster.h, built by plain g++),
with identical positional arguments and return tuples; this file loads it and fails loudly when it (or libtgs_raster.so) cannot be
built or loaded.  The batch / introspection / test entry points that have no counterpart in the reference are thin ctypes bindings of the
same C ABI.  Torch supplies device memory and the current HIP stream, nothing else.  There is NO CPU fallback: tensors that are not on a
HIP device are rejected.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

from .. import build as _build

_LIB_PATH = os.environ.get("TGS_LIBRARY") or _build.LIB       # TGS_LIBRARY: another build of the same ABI (A/B measurements on one box)


ABI_VERSION = 3                # TGS_ABI_VERSION of include/tgs_raster.h this binding is written against


def _load() -> C.CDLL:
    if "TGS_LIBRARY" not in os.environ:
        try:
            _build.build_native()       # no-op when the library is newer than csrc/*.hip and tgs_raster.h: never run stale kernels
        except Exception as e:  # loud: no silent fallback -- neither to a CPU path nor to a library older than its sources
            what = "is older than its sources" if os.path.exists(_LIB_PATH) else "is missing"
            raise ImportError(f"libtgs_raster.so {what} and could not be rebuilt ({e}); run "
                              f"`python -c 'import __graft_entry__ as g; g.build()'` on a ROCm machine") from e
    lib = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)        # the compiled _Cext resolves its tgs_* symbols against this very library
    vp, fl, it = C.c_void_p, C.c_float, C.c_int
    lib.tgs_abi_version.restype = it
    if lib.tgs_abi_version() != ABI_VERSION:
        raise ImportError(f"libtgs_raster.so has ABI version {lib.tgs_abi_version()}, this binding needs {ABI_VERSION}: rebuild it "
                          "(`python -m youreditableavatar_amd.build --force`)")
    lib.tgs_sizeof_view.restype = C.c_size_t
    lib.tgs_sizeof_options.restype = C.c_size_t
    lib.tgs_last_error.restype = C.c_char_p
    lib.tgs_frame_status.restype = it
    lib.tgs_frame_status.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(it)]
    lib.tgs_state_sizes.restype = None
    lib.tgs_state_sizes.argtypes = [it, it, it, it, it, C.c_int64, C.POINTER(C.c_size_t)]
    lib.tgs_set_render_streams.restype = it
    lib.tgs_set_render_streams.argtypes = [vp, it]
    lib.tgs_forward_views_opt.restype = it
    lib.tgs_forward_views_opt.argtypes = [vp, vp, it, C.c_int64, it, it, it, vp, vp, vp, vp, vp, fl, vp, vp, it, it, vp]
    lib.tgs_backward_render_views_opt.restype = it
    lib.tgs_backward_render_views_opt.argtypes = [vp, vp, it, it, it, vp]
    lib.tgs_backward_render_opt.restype = it
    lib.tgs_backward_render_opt.argtypes = [vp, vp, it, C.c_int64, vp, it, it, vp, vp, vp]
    try:                                                     # (additive: an older A/B build of the same ABI version lacks it)
        lib.tgs_backward_render_alpha_opt.restype = it
        lib.tgs_backward_render_alpha_opt.argtypes = lib.tgs_backward_render_opt.argtypes + [vp]
    except AttributeError:
        pass
    lib.tgs_backward_batch.restype = it
    lib.tgs_backward_batch.argtypes = [vp, it, it, it, it, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, vp, vp, vp, it]
    lib.tgs_backward_batch_range.restype = it
    lib.tgs_backward_batch_range.argtypes = lib.tgs_backward_batch.argtypes + [it, it]
    try:                                                     # (additive since round 6: an older A/B build of the same ABI version lacks it)
        lib.tgs_backward_batch_range_planes.restype = it
        lib.tgs_backward_batch_range_planes.argtypes = lib.tgs_backward_batch_range.argtypes + [C.c_int64]
    except AttributeError:
        pass
    # alpha and depth in the whole-batch path (tgs_view_extras_t): part of this binding, so a library without them is stale
    lib.tgs_sizeof_view_extras.restype = C.c_size_t
    lib.tgs_outputs_views.restype = it
    lib.tgs_outputs_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_render_views_extras_opt.restype = it
    lib.tgs_backward_render_views_extras_opt.argtypes = [vp, vp, it, it, it, vp, vp]
    lib.tgs_backward_batch_depth_range.restype = it
    lib.tgs_backward_batch_depth_range.argtypes = [vp, it, it, vp, vp, vp, it, it]
    # feature channels in the whole-batch path (tgs_view_features_t)
    lib.tgs_sizeof_view_features.restype = C.c_size_t
    lib.tgs_features_views.restype = it
    lib.tgs_features_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_render_views_features_opt.restype = it
    lib.tgs_backward_render_views_features_opt.argtypes = [vp, vp, it, it, it, vp, vp, vp]
    lib.tgs_backward_batch_features_range.restype = it
    lib.tgs_backward_batch_features_range.argtypes = [vp, it, it, vp, vp, vp, it, it, it]
    # median depth of one view: the map and the call that adds its share behind a backward
    lib.tgs_median.restype = it
    lib.tgs_median.argtypes = [vp, it, it, it, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.tgs_backward_median.restype = it
    lib.tgs_backward_median.argtypes = [vp, it, it, it, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # the median of a batch's views (tgs_view_median_t) and the surface votes over their index maps
    try:                                                     # (additive: an older A/B build of the same ABI version, TGS_LIBRARY, lacks them -- calling one raises)
        lib.tgs_sizeof_view_median.restype = C.c_size_t
        lib.tgs_median_views.restype = it
        lib.tgs_median_views.argtypes = [vp, it, it, it, vp, vp]
        lib.tgs_backward_median_views.restype = it
        lib.tgs_backward_median_views.argtypes = [vp, it, it, it, vp, vp]
        lib.tgs_backward_batch_median_range.restype = it
        lib.tgs_backward_batch_median_range.argtypes = [vp, it, it, vp, vp, vp, it, it]
        lib.tgs_surface_votes.restype = it
        lib.tgs_surface_votes.argtypes = [vp, it, C.c_int64, vp, vp, vp, vp]
    except AttributeError:
        if "TGS_LIBRARY" not in os.environ:
            raise
    lib.tgs_state_field.restype = C.c_int64
    lib.tgs_state_field.argtypes = [vp, C.c_char_p, it, it, it, C.c_int64, it, it, vp, vp, vp, vp, C.c_size_t]
    lib.tgs_set_sort_lds_cap.restype = it
    lib.tgs_set_sort_lds_cap.argtypes = [C.c_uint]
    lib.tgs_set_instance_pruning.restype = None
    lib.tgs_set_instance_pruning.argtypes = [it]
    lib.tgs_set_forward_group.restype = None
    lib.tgs_set_forward_group.argtypes = [it]
    lib.tgs_last_nonempty_tiles.restype = C.c_int64
    lib.tgs_last_nonempty_tiles.argtypes = []
    lib.tgs_set_deterministic.restype = None
    lib.tgs_set_deterministic.argtypes = [it]
    lib.tgs_selftest_reduce36.restype = it
    lib.tgs_selftest_reduce36.argtypes = [vp, vp, vp]
    lib.tgs_profile_begin.restype = it
    lib.tgs_profile_begin.argtypes = [it]
    lib.tgs_profile_stages.restype = None
    lib.tgs_profile_stages.argtypes = [C.c_uint]
    lib.tgs_profile_end.restype = it
    lib.tgs_profile_end.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    return lib


_lib = _load()


def _load_ext():
    """The compiled glue module.  Built on demand (g++, ~40 s) when missing or older than its source; an ImportError otherwise."""
    import importlib
    try:
        _build.build_torch_ext()
    except Exception as e:
        what = "is older than its sources" if os.path.exists(_build.ext_path()) else "is missing"
        raise ImportError(f"the compiled _C extension ({_build.EXT_NAME}) {what} and could not be rebuilt ({e}); run "
                          f"`python -c 'import __graft_entry__ as g; g.build()'`") from e
    ext = importlib.import_module(__package__ + "." + _build.EXT_NAME)
    if ext.abi_version() != ABI_VERSION or ext.compiled_abi_version() != ABI_VERSION:
        raise ImportError(f"compiled _C extension: ABI version {ext.compiled_abi_version()} (library {ext.abi_version()}), this binding needs {ABI_VERSION}")
    return ext


_ext = _load_ext()
STAGES = ("preprocess_fwd", "scan", "scatter", "tile_sort", "render_fwd", "render_bwd", "preprocess_bwd")


# ---- test-only shims (include/tgs_raster_testing.h): process-wide DEFAULTS for calls made without explicit options.  Every entry point of this
# module passes an explicit tgs_options_t (options(...)); a field left at None / 0 there falls back to what these setters stored.  There is no
# shim for the tile bound any more: with explicit options a tile_bound of 0 means "none", so a thread-wide default could never take effect
# through these bindings -- pass tile_bound= to the call.
def set_sort_lds_cap(cap: int) -> None:
    """Test knob: tile lists longer than ``cap`` (power of two <= 8192) take the global-memory sort path."""
    if _lib.tgs_set_sort_lds_cap(int(cap)) < 0:
        raise _err(-1)


def set_instance_pruning(on: bool) -> None:
    """False: keep the reference's tile instances (every tile of the 3-sigma rectangle); True (default): drop those that cannot
    reach alpha >= 1/255 anywhere in the tile.  Same images and gradients either way."""
    _lib.tgs_set_instance_pruning(1 if on else 0)


def set_forward_group(views_per_launch: int) -> None:
    """Views per launch of the per-Gaussian forward stage inside forward_views (1..8; default 1)."""
    _lib.tgs_set_forward_group(int(views_per_launch))


def last_nonempty_tiles() -> int:
    """Tiles with instances of the last frame this thread rendered with the synchronous or the speculative forward (-1: unknown)."""
    return int(_lib.tgs_last_nonempty_tiles())


def set_deterministic(on: bool) -> None:
    """True: bitwise-reproducible backward (fixed in-tile summation order, slower); False: default."""
    _lib.tgs_set_deterministic(1 if on else 0)


def selftest_reduce36(x: torch.Tensor) -> torch.Tensor:
    """x[64,36] on the GPU -> [4,9] sums over the wave (checks the permlane-swap reduction on hardware)."""
    x = x.contiguous().float()
    out = torch.empty((4, 9), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        if _lib.tgs_selftest_reduce36(torch.cuda.current_stream(x.device).cuda_stream, x.data_ptr(), out.data_ptr()) < 0:
            raise RuntimeError("selftest launch failed")
    return out


def profile_begin(max_records: int = 100000, stages=None) -> None:
    """Bench instrumentation: hipEvents around the pipeline stages (all, or the names in ``stages``) on the caller's
    stream (no syncs)."""
    mask = 0xffffffff if stages is None else sum(1 << STAGES.index(n) for n in stages)
    _lib.tgs_profile_stages(mask)
    if _lib.tgs_profile_begin(int(max_records)) < 0:
        raise RuntimeError("profiling already active")


def profile_end():
    """-> {stage: (total_ms, launches)}; waits for the recorded events."""
    ms = (C.c_double * len(STAGES))()
    cnt = (C.c_int64 * len(STAGES))()
    if _lib.tgs_profile_end(ms, cnt) < 0:
        raise RuntimeError("profiling not active")
    return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(STAGES)}


class _OptionsT(C.Structure):
    """tgs_options_t (include/tgs_raster.h): everything that tunes one call, passed explicitly -- nothing process-wide is touched"""
    _fields_ = [("struct_size", C.c_uint32), ("instance_pruning", C.c_int32), ("deterministic", C.c_int32), ("forward_group", C.c_int32),
                ("sort_lds_cap", C.c_uint32), ("tile_bound", C.c_int64), ("heavy_bound", C.c_int64), ("mid_bound", C.c_int64),
                ("light_tiles", C.c_int32)]


def options(tile_bound: int = 0, pruning: Optional[bool] = None, deterministic: Optional[bool] = None, forward_group: int = 0, sort_lds_cap: int = 0,
            light_tiles: Optional[bool] = None, mid_bound: int = 0, heavy_bound: int = 0) -> _OptionsT:
    """A filled tgs_options_t (None / 0: the library default of that field)."""
    o = _OptionsT()
    o.struct_size = C.sizeof(_OptionsT)
    o.instance_pruning = -1 if pruning is None else int(bool(pruning))
    o.deterministic = -1 if deterministic is None else int(bool(deterministic))
    o.forward_group, o.sort_lds_cap = int(forward_group), int(sort_lds_cap)
    o.tile_bound, o.mid_bound, o.heavy_bound = max(0, int(tile_bound)), max(0, int(mid_bound)), max(0, int(heavy_bound))
    o.light_tiles = -1 if light_tiles is None else int(bool(light_tiles))
    return o


def loaded_library() -> str:
    """Path of the native library this process is using (for diagnostics)."""
    return _LIB_PATH


def _err(code: int) -> RuntimeError:
    msg = _lib.tgs_last_error()
    return RuntimeError(f"{msg.decode() if msg else 'tgs_raster error'} (code {code})")


def _dev_f32(t: torch.Tensor, dev: torch.device, name: str) -> Optional[torch.Tensor]:
    """contiguous fp32 tensor on ``dev``; an empty tensor is the reference's 'absent' (NULL)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float but found {t.dtype} for {name}")
    if t.device != dev:
        t = t.to(dev)
    return t.contiguous()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _require_gpu(means3D: torch.Tensor) -> torch.device:
    if not means3D.is_cuda:
        raise RuntimeError("diff_gaussian_rasterization (MI355X build) has no CPU path: means3D must be on a HIP device")
    return means3D.device


META_BYTES = 64
FRAME_PREFILTERED, FRAME_REJECTED = 1, 2


def frame_meta(image_buffer: torch.Tensor) -> torch.Tensor:
    """The frame's 64-byte Meta record (a view of the image buffer, on the device): gather these for a batch of
    sync-free frames and decode them on the host with ``decode_meta`` after ONE copy."""
    return image_buffer[:META_BYTES]


def decode_meta_full(meta_bytes: torch.Tensor) -> Tuple[int, int, int, int]:
    """64 Meta bytes on the host -> (num_rendered, flags, longest tile list, tiles beyond the LDS sort).  In a record the scan kernel wrote
    to pinned memory itself (tgs_view_t.host_meta) the word at byte 32 says that a tile bound was exceeded: folded into FRAME_REJECTED."""
    import struct
    raw = bytes(meta_bytes.cpu().numpy().tobytes())
    R, max_count, n_overflow, flags = struct.unpack_from("<QIII", raw, 0)
    if struct.unpack_from("<I", raw, 32)[0]:
        flags |= FRAME_REJECTED
    return int(R), int(flags), int(max_count), int(n_overflow)


def decode_meta_tiles(meta_bytes: torch.Tensor) -> Tuple[int, int, int]:
    """64 Meta bytes on the host -> tiles that hold instances, tiles with >= 1024 of them, tiles with >= 128."""
    import struct
    n, heavy, mid = struct.unpack_from("<III", bytes(meta_bytes.cpu().numpy().tobytes()), 20)
    return int(n), int(heavy), int(mid)


def decode_meta(meta_bytes: torch.Tensor) -> Tuple[int, int]:
    """64 Meta bytes on the host -> (num_rendered, flags)."""
    R, flags, _m, _o = decode_meta_full(meta_bytes)
    return R, flags


def frame_status(image_buffer: torch.Tensor) -> Tuple[int, int]:
    """tgs_frame_status: synchronises the current stream; -> (true num_rendered, TGS_FRAME_* flags)."""
    dev = image_buffer.device
    R, fl = C.c_int64(0), C.c_int(0)
    with torch.cuda.device(dev):
        r = _lib.tgs_frame_status(torch.cuda.current_stream(dev).cuda_stream, image_buffer.data_ptr(), C.byref(R), C.byref(fl))
    if r < 0:
        raise _err(int(r))
    return int(R.value), int(fl.value)


def rasterize_gaussians_backward_accumulate(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                            viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                                            geomBuffer, R, binningBuffer, imageBuffer, debug, into, tile_bound: int = 0,
                                            deterministic: Optional[bool] = None, mid_bound: int = 0, *,
                                            grad_out_alpha: Optional[torch.Tensor] = None, grad_out_depth: Optional[torch.Tensor] = None,
                                            grad_out_features: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None,
                                            grad_out_median: Optional[torch.Tensor] = None, median_pos: Optional[torch.Tensor] = None):
    """Multi-view extension (tgs_backward_accumulate): parameter gradients are ADDED into the fp32 tensors of ``into``
    (keys: means3D, opacities, and sh|colors_precomp, scales+rotations|cov3D_precomp; contiguous, on the device).
    Returns dL_dmeans2D[P,3], the only per-view gradient.  ``grad_out_alpha`` / ``grad_out_depth`` ([1,H,W]): upstream gradients of the
    frame's accumulated alpha / expected depth as well (the library's depth call with accumulate = 1; the dz scratch of R floats is
    allocated by the binding); both None: the plain accumulating call, bit for bit.  ``grad_out_features`` ([C,H,W]) with ``features``
    ([P,C], float32, 1 <= C <= 16): the upstream gradient of the frame's feature map as well (the library's feature call with accumulate = 1;
    the scratch of R * C floats is allocated by the binding); dL/d features is ADDED into ``into["features"]`` ([P,C]), which is required then.
    ``grad_out_median`` ([1,H,W]) with ``median_pos`` (the int32 map [1,H,W] of ``median_from_state`` for this frame): the upstream gradient
    of the frame's median depth as well -- tgs_backward_median behind the main call adds its share into ``into["means3D"]`` (its scratch of R
    floats is the depth's where there is one); no other gradient gets anything from it.  None: today's calls and today's kernels.
    A forward to the compiled ``rasterize_gaussians_backward_into``: the implementation ``rasterize_gaussians_backward`` stores through."""
    return _ext.rasterize_gaussians_backward_into(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                                  tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, into,
                                                  tile_bound, deterministic, mid_bound, grad_out_alpha, grad_out_depth, grad_out_features, features,
                                                  grad_out_median, median_pos)


class _ViewT(C.Structure):
    """tgs_view_t (include/tgs_raster.h)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p), ("radii", C.c_void_p),
                ("geom_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("img_buffer", C.c_void_p), ("R", C.c_int64),
                ("dL_dmean2D", C.c_void_p), ("dL_dcolor", C.c_void_p),
                ("background", C.c_void_p), ("out_color", C.c_void_p), ("radii_out", C.c_void_p), ("dL_dpix", C.c_void_p),
                ("geom_bytes", C.c_size_t), ("binning_bytes", C.c_size_t), ("img_bytes", C.c_size_t), ("colors_precomp", C.c_void_p),
                ("tile_bound", C.c_int64), ("heavy_bound", C.c_int64), ("mid_bound", C.c_int64), ("host_meta", C.c_void_p)]


if _lib.tgs_sizeof_view() != C.sizeof(_ViewT) or _ext.sizeof_view() != C.sizeof(_ViewT) or _lib.tgs_sizeof_options() != C.sizeof(_OptionsT):
    raise ImportError(f"tgs_view_t / tgs_options_t: the library says {_lib.tgs_sizeof_view()} / {_lib.tgs_sizeof_options()} bytes, this binding declares "
                      f"{C.sizeof(_ViewT)} / {C.sizeof(_OptionsT)} -- a stale library or binding")
ViewArray = lambda n: (_ViewT * n)()


class _ViewExtrasT(C.Structure):
    """tgs_view_extras_t (include/tgs_raster.h): alpha / depth outputs and gradients of one view, beside its tgs_view_t"""
    _fields_ = [("struct_size", C.c_uint32), ("out_alpha", C.c_void_p), ("out_depth", C.c_void_p), ("dL_dalpha", C.c_void_p),
                ("dL_ddepth", C.c_void_p), ("dz_scratch", C.c_void_p)]


if _lib.tgs_sizeof_view_extras() != C.sizeof(_ViewExtrasT):
    raise ImportError(f"tgs_view_extras_t: the library says {_lib.tgs_sizeof_view_extras()} bytes, this binding declares {C.sizeof(_ViewExtrasT)} "
                      "-- a stale library or binding")


def ViewExtrasArray(n: int):
    """n zeroed tgs_view_extras_t with struct_size set (every pointer NULL: nothing asked of any view)"""
    arr = (_ViewExtrasT * n)()
    for x in arr:
        x.struct_size = C.sizeof(_ViewExtrasT)
    return arr


class _ViewFeaturesT(C.Structure):
    """tgs_view_features_t (include/tgs_raster.h): the feature map and its gradient of one view, beside its tgs_view_t and tgs_view_extras_t"""
    _fields_ = [("struct_size", C.c_uint32), ("C", C.c_int32), ("features", C.c_void_p), ("out_features", C.c_void_p),
                ("dL_dfeature_map", C.c_void_p), ("feature_scratch", C.c_void_p)]


if _lib.tgs_sizeof_view_features() != C.sizeof(_ViewFeaturesT) or _ext.sizeof_view_features() != C.sizeof(_ViewFeaturesT):
    raise ImportError(f"tgs_view_features_t: the library says {_lib.tgs_sizeof_view_features()} bytes, this binding declares {C.sizeof(_ViewFeaturesT)} "
                      "-- a stale library or binding")


def ViewFeaturesArray(n: int):
    """n zeroed tgs_view_features_t with struct_size set (C = 0 and every pointer NULL: nothing asked of any view)"""
    arr = (_ViewFeaturesT * n)()
    for x in arr:
        x.struct_size = C.sizeof(_ViewFeaturesT)
    return arr


class _ViewMedianT(C.Structure):
    """tgs_view_median_t (include/tgs_raster.h): the median maps and the median depth's gradient of one view, the fourth per-view array"""
    _fields_ = [("struct_size", C.c_uint32), ("out_depth", C.c_void_p), ("out_index", C.c_void_p), ("out_pos", C.c_void_p),
                ("dL_dmedian_depth", C.c_void_p), ("dz_scratch", C.c_void_p)]


if hasattr(_lib, "tgs_sizeof_view_median") and _lib.tgs_sizeof_view_median() != C.sizeof(_ViewMedianT):
    raise ImportError(f"tgs_view_median_t: the library says {_lib.tgs_sizeof_view_median()} bytes, this binding declares {C.sizeof(_ViewMedianT)} "
                      "-- a stale library or binding")


def ViewMedianArray(n: int):
    """n zeroed tgs_view_median_t with struct_size set (every pointer NULL: nothing asked of any view)"""
    arr = (_ViewMedianT * n)()
    for x in arr:
        x.struct_size = C.sizeof(_ViewMedianT)
    return arr


def state_sizes(P: int, width: int, height: int, has_sh: bool, has_scale_rot: bool, r_capacity: int) -> Tuple[int, int, int]:
    """tgs_state_sizes -> bytes of the (geometry, binning, image) state buffers of one view."""
    out = (C.c_size_t * 3)()
    _lib.tgs_state_sizes(int(P), int(width), int(height), int(bool(has_sh)), int(bool(has_scale_rot)), int(r_capacity), out)
    return int(out[0]), int(out[1]), int(out[2])


_NO_OPTIONS = object()                  # (a *_views function of the library without an options parameter)


def _ptr(a):
    """a ctypes array (views, extras, feats) as the pointer the library takes; None and pointers stay"""
    return a if a is None or isinstance(a, C.c_void_p) else C.cast(a, C.c_void_p)


def _views_call(fn, opt, stream_handles, *args):
    """One *_views call of the library: ``opt`` by reference (None: NULL; _NO_OPTIONS: ``fn`` takes none), the stream handles as an array and
    their number, then ``args``; an error code raises.  (This sits in every step of the whole-batch path, several times: a few microseconds
    of Python per call show in bench.py, so the arguments come converted and nothing here loops over them.)"""
    arr = (C.c_void_p * len(stream_handles))(*stream_handles)
    if opt is _NO_OPTIONS:
        r = fn(arr, len(stream_handles), *args)
    else:
        r = fn(C.byref(opt) if opt is not None else None, arr, len(stream_handles), *args)
    if r < 0:
        raise _err(int(r))


def forward_views(stream_handles, r_capacity, P, D, M, means3D, shs, opacities, scales, scale_modifier, rotations, views, n_views, prefiltered=False,
                  opt: Optional[_OptionsT] = None) -> None:
    """tgs_forward_views_opt on prepared device pointers (ints) and a filled ``ViewArray``; ``opt``: ``options(...)`` or None (defaults)."""
    _views_call(_lib.tgs_forward_views_opt, opt, stream_handles, int(r_capacity), int(P), int(D), int(M), means3D, shs, None, opacities, scales, float(scale_modifier),
                rotations, None, int(bool(prefiltered)), int(n_views), _ptr(views))


def set_render_streams(stream_handles) -> None:
    """tgs_set_render_streams: later forward_views calls of this thread put k_render_fwd of view k on stream_handles[k mod n] ([] resets)."""
    arr = (C.c_void_p * max(1, len(stream_handles)))(*stream_handles)
    _lib.tgs_set_render_streams(arr, len(stream_handles))


def backward_render_views(stream_handles, P, views, n_views, opt: Optional[_OptionsT] = None) -> None:
    _views_call(_lib.tgs_backward_render_views_opt, opt, stream_handles, int(P), int(n_views), _ptr(views))


def outputs_views(stream_handles, P, views, extras, n_views) -> None:
    """tgs_outputs_views: alpha / depth of every view into extras[k].out_alpha / out_depth; ``stream_handles``: the streams the views'
    k_render_fwd ran on (forward_views' streams, or the render streams when set_render_streams was in force)."""
    _views_call(_lib.tgs_outputs_views, _NO_OPTIONS, stream_handles, int(P), int(n_views), _ptr(views), _ptr(extras))


def backward_render_views_extras(stream_handles, P, views, extras, n_views, opt: Optional[_OptionsT] = None) -> None:
    """tgs_backward_render_views_extras_opt: backward_render_views with extras[k].dL_dalpha / dL_ddepth entering view k's per-pixel backward."""
    _views_call(_lib.tgs_backward_render_views_extras_opt, opt, stream_handles, int(P), int(n_views), _ptr(views), _ptr(extras))


def backward_batch_depth_raw(stream, P, views, extras, n_views, dL_dmean3D, first: int = 0, count: Optional[int] = None) -> None:
    """tgs_backward_batch_depth_range: the z-path of the depth gradient of all views, added to dL_dmean3D (a device pointer) for Gaussians
    [first, first + count) -- behind the backward_batch_raw call of the same range, on the same stream."""
    r = _lib.tgs_backward_batch_depth_range(stream, int(P), int(n_views), C.cast(views, C.c_void_p), C.cast(extras, C.c_void_p), dL_dmean3D,
                                            int(first), int(P - first if count is None else count))
    if r < 0:
        raise _err(int(r))


def features_views(stream_handles, P, views, feats, n_views) -> None:
    """tgs_features_views: the feature map of every view into feats[k].out_features; ``stream_handles``: as for ``outputs_views``, the streams
    the views' k_render_fwd ran on."""
    _views_call(_lib.tgs_features_views, _NO_OPTIONS, stream_handles, int(P), int(n_views), _ptr(views), _ptr(feats))


def backward_render_views_features(stream_handles, P, views, extras, feats, n_views, opt: Optional[_OptionsT] = None) -> None:
    """tgs_backward_render_views_features_opt: backward_render_views_extras (``extras`` may be None) with feats[k].dL_dfeature_map entering
    view k's per-pixel backward behind the depth's share; the channel sums stay in feats[k].feature_scratch."""
    _views_call(_lib.tgs_backward_render_views_features_opt, opt, stream_handles, int(P), int(n_views), _ptr(views), _ptr(extras), _ptr(feats))


def backward_batch_features_raw(stream, P, views, feats, n_views, dL_dfeatures, accumulate, first: int = 0, count: Optional[int] = None) -> None:
    """tgs_backward_batch_features_range: dL/d features of all views, stored (``accumulate`` false) or added into dL_dfeatures (a device
    pointer, [P,C]) for Gaussians [first, first + count) -- on the stream of the backward_batch_raw call of the same range."""
    r = _lib.tgs_backward_batch_features_range(stream, int(P), int(n_views), C.cast(views, C.c_void_p), C.cast(feats, C.c_void_p), dL_dfeatures,
                                               1 if accumulate else 0, int(first), int(P - first if count is None else count))
    if r < 0:
        raise _err(int(r))


def median_views(stream_handles, P, views, med, n_views) -> None:
    """tgs_median_views: median depth, surface index and list position of every view whose med[k] has the three output pointers, from the
    frames of a finished forward_views call; view k on stream_handles[k mod n] -- streams ordered behind the views' k_render_fwd."""
    _views_call(_lib.tgs_median_views, _NO_OPTIONS, stream_handles, int(P), int(n_views), _ptr(views), _ptr(med))


def backward_median_views(stream_handles, P, views, med, n_views) -> None:
    """tgs_backward_median_views: per view with med[k].dL_dmedian_depth, the upstream gradients of the pixels that share a median entry summed
    into med[k].dz_scratch (out_pos: the map median_views wrote for the same frames).  The per-Gaussian half is backward_batch_median_raw."""
    _views_call(_lib.tgs_backward_median_views, _NO_OPTIONS, stream_handles, int(P), int(n_views), _ptr(views), _ptr(med))


def backward_batch_median_raw(stream, P, views, med, n_views, dL_dmean3D, first: int = 0, count: Optional[int] = None) -> None:
    """tgs_backward_batch_median_range: the median depth's gradient of all views, ADDED to dL_dmean3D (a device pointer) for Gaussians
    [first, first + count) -- on one stream, behind backward_median_views on every lane and behind whatever wrote dL_dmean3D."""
    r = _lib.tgs_backward_batch_median_range(stream, int(P), int(n_views), C.cast(views, C.c_void_p), C.cast(med, C.c_void_p), dL_dmean3D,
                                             int(first), int(P - first if count is None else count))
    if r < 0:
        raise _err(int(r))


def backward_median_raw(stream, P, W, H, R, geom, binning, img, viewmatrix, radii, median_pos, dL_dmedian_depth, dz_scratch, dL_dmean3D) -> None:
    """tgs_backward_median on device pointers: one view's median gradient ADDED to dL_dmean3D, on ``stream``."""
    r = _lib.tgs_backward_median(stream, int(P), int(W), int(H), int(R), geom, binning, img, viewmatrix, radii, median_pos, dL_dmedian_depth, dz_scratch, dL_dmean3D)
    if r < 0:
        raise _err(int(r))


def surface_votes(index: torch.Tensor, P: int, mask: Optional[torch.Tensor] = None, out=None):
    """tgs_surface_votes over the pixels of ``index`` (int32, any shape, contiguous, on a HIP device): -> (seen[P], hits[P] or None), int32:
    seen[p] += pixels whose index is p, hits[p] += those of them whose ``mask`` (uint8 or bool, as many elements as ``index``) is not zero.
    ``out=(seen, hits)``: int32 [P] tensors that are ADDED to (hits may be None without a mask); otherwise new zeroed ones.  On the current
    stream; nothing is read back."""
    if not (torch.is_tensor(index) and index.is_cuda and index.dtype == torch.int32 and index.is_contiguous()):
        raise RuntimeError("surface_votes: index must be a contiguous int32 tensor on a HIP device")
    dev, P = index.device, int(P)
    if P < 0:
        raise RuntimeError("surface_votes: P must not be negative")
    if mask is not None:
        if not (torch.is_tensor(mask) and mask.device == dev and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and
                mask.numel() == index.numel()):
            raise RuntimeError("surface_votes: mask must be a contiguous uint8 or bool tensor on the device of index, with as many elements")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)                    # (a bool is one byte, 0 or 1: the same storage)
    with torch.cuda.device(dev):
        if out is None:
            seen = torch.zeros(P, dtype=torch.int32, device=dev)
            hits = torch.zeros(P, dtype=torch.int32, device=dev) if mask is not None else None
        else:
            seen, hits = out
            for name, t in (("seen", seen), ("hits", hits)):
                if t is None and (name == "hits" and mask is None):
                    continue
                if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (P,)):
                    raise RuntimeError(f"surface_votes: out {name} must be a contiguous int32 tensor [P] on the device of index")
            if mask is None:
                hits = None
        r = _lib.tgs_surface_votes(torch.cuda.current_stream(dev).cuda_stream, P, int(index.numel()), index.data_ptr(), _p(mask), seen.data_ptr(), _p(hits))
    if r < 0:
        raise _err(int(r))
    return seen, hits


def backward_batch_raw(stream, P, D, M, views, n_views, means3D, shs, scales, scale_modifier, rotations, dL_dopacity, dL_dmean3D, dL_dsh, dL_dscale,
                       dL_drot, accumulate, first: int = 0, count: Optional[int] = None, dsh_plane_stride: int = 0) -> None:
    """tgs_backward_batch[_range] on prepared device pointers (scales/rotations path; ``shs`` None: per-view colours, their gradients go to
    the views' dL_dcolor).  ``first`` / ``count``: only Gaussians [first, first + count) (multiples of 256, or ending at P).
    ``dsh_plane_stride`` > 0: dL_dsh level-major (tgs_backward_batch_range_planes: coefficient k of Gaussian p at k * stride + 3 p)."""
    args = (stream, int(P), int(D), int(M), int(n_views), views if isinstance(views, C.c_void_p) else C.cast(views, C.c_void_p), means3D, shs,
            scales, float(scale_modifier),
            rotations, None, dL_dopacity, dL_dmean3D, None, dL_dsh if shs else None, dL_dscale, dL_drot, 1 if accumulate else 0,
            int(first), int(P - first if count is None else count))
    r = _lib.tgs_backward_batch_range_planes(*args, int(dsh_plane_stride)) if dsh_plane_stride else _lib.tgs_backward_batch_range(*args)
    if r < 0:
        raise _err(int(r))


def rasterize_gaussians_backward_render(background, dL_dout_color, R, binningBuffer, imageBuffer, P, tile_bound: int = 0,
                                        deterministic: Optional[bool] = None, grad_out_alpha: Optional[torch.Tensor] = None) -> None:
    """tgs_backward_render: the per-pixel half of one view's backward; the tile partials stay in ``binningBuffer`` for
    ``rasterize_gaussians_backward_batch``.  ``grad_out_alpha`` ([1,H,W]): upstream gradient of the accumulated alpha as well
    (tgs_backward_render_alpha_opt); None: today's call."""
    dev = _require_gpu(dL_dout_color)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    with torch.cuda.device(dev):
        bg, dL = _dev_f32(background, dev, "background"), _dev_f32(dL_dout_color, dev, "dL_dout_color")
        opt = options(tile_bound=tile_bound, deterministic=deterministic)
        if grad_out_alpha is not None:
            if grad_out_alpha.numel() != H * W:
                raise RuntimeError("grad_out_alpha must have H*W elements ([1,H,W])")
            dA = _dev_f32(grad_out_alpha, dev, "grad_out_alpha")
            r = _lib.tgs_backward_render_alpha_opt(C.byref(opt), torch.cuda.current_stream(dev).cuda_stream, int(P), int(R), _p(bg), W, H,
                                                   binningBuffer.data_ptr(), imageBuffer.data_ptr(), _p(dL), _p(dA))
        else:
            r = _lib.tgs_backward_render_opt(C.byref(opt), torch.cuda.current_stream(dev).cuda_stream, int(P), int(R), _p(bg), W, H, binningBuffer.data_ptr(),
                                             imageBuffer.data_ptr(), _p(dL))
    if r < 0:
        raise _err(int(r))


def rasterize_gaussians_backward_batch(views, means3D, sh, degree, scales, rotations, scale_modifier, cov3D_precomp, into, accumulate=True):
    """tgs_backward_batch: the per-Gaussian half for all ``views`` of a batch in one pass.

    ``views``: dicts with keys viewmatrix, projmatrix, campos, tanfovx, tanfovy, image_height, image_width, radii, geom, binning, img,
    R (and colors=True on the colors_precomp path).  Parameter gradients are stored (``accumulate=False``) or added into the tensors
    of ``into`` (keys: means3D, opacities, and sh, scales + rotations | cov3D_precomp).  Returns, per view, dL_dmeans2D[P,3]
    (and dL_dcolors[P,3] on the colors_precomp path)."""
    dev = _require_gpu(means3D)
    P = int(means3D.size(0))
    M = int(sh.size(1)) if (sh is not None and sh.dim() > 1 and sh.size(0) != 0) else 0
    has_sh = M > 0
    outs = []
    if P == 0 or not views:
        return outs
    with torch.cuda.device(dev):
        t = dict(means=_dev_f32(means3D, dev, "means3D"), sh=_dev_f32(sh, dev, "sh") if has_sh else None, scales=_dev_f32(scales, dev, "scales"),
                 rots=_dev_f32(rotations, dev, "rotations"), cov=_dev_f32(cov3D_precomp, dev, "cov3D_precomp"))
        has_sr = t["scales"] is not None
        arr = (_ViewT * len(views))()
        keep = []
        for i, v in enumerate(views):
            vm, pm, cp = _dev_f32(v["viewmatrix"], dev, "viewmatrix"), _dev_f32(v["projmatrix"], dev, "projmatrix"), _dev_f32(v["campos"], dev, "campos")
            radii = v["radii"].contiguous()
            g2d = torch.empty((P, 3), dtype=torch.float32, device=dev)
            gcol = None if has_sh else torch.empty((P, 3), dtype=torch.float32, device=dev)
            keep += [vm, pm, cp, radii]
            a = arr[i]
            a.width, a.height, a.tan_fovx, a.tan_fovy = int(v["image_width"]), int(v["image_height"]), float(v["tanfovx"]), float(v["tanfovy"])
            a.viewmatrix, a.projmatrix, a.campos, a.radii = vm.data_ptr(), pm.data_ptr(), cp.data_ptr(), radii.data_ptr()
            a.geom_buffer, a.binning_buffer, a.img_buffer, a.R = v["geom"].data_ptr(), v["binning"].data_ptr(), v["img"].data_ptr(), int(v["R"])
            a.dL_dmean2D, a.dL_dcolor = g2d.data_ptr(), (gcol.data_ptr() if gcol is not None else None)
            outs.append((g2d, gcol))

        def dst(name, shape):
            g = into.get(name)
            if g is None:
                raise RuntimeError(f"rasterize_gaussians_backward_batch: no gradient buffer for {name}")
            if g.dtype != torch.float32 or g.device != dev or not g.is_contiguous() or tuple(g.shape) != shape:
                raise RuntimeError(f"gradient buffer for {name} must be a contiguous fp32 tensor of shape {shape} on {dev}")
            return g.data_ptr()

        r = _lib.tgs_backward_batch(torch.cuda.current_stream(dev).cuda_stream, P, int(degree), M, len(views), C.cast(arr, C.c_void_p), _p(t["means"]),
                                    _p(t["sh"]), _p(t["scales"]), float(scale_modifier), _p(t["rots"]), _p(t["cov"]), dst("opacities", (P, 1)),
                                    dst("means3D", (P, 3)), None if has_sr else dst("cov3D_precomp", (P, 6)), dst("sh", (P, M, 3)) if has_sh else None,
                                    dst("scales", (P, 3)) if has_sr else None, dst("rotations", (P, 4)) if has_sr else None, 1 if accumulate else 0)
        del keep
    if r < 0:
        raise _err(int(r))
    return outs


_FIELD_DTYPES = {"n_contrib": torch.int32, "final_T": torch.float32, "ranges": torch.int32, "point_list": torch.int32, "block_masks": torch.int32,
                 "means2D": torch.float32, "depths": torch.float32, "conic_opacity": torch.float32, "rgb": torch.float32,
                 "tiles_touched": torch.int32, "tile_order": torch.int32, "stamps": torch.int64, "quad_masks": torch.int64}


def state_field(name: str, P: int, width: int, height: int, R: int, has_sh: bool, has_scale_rot: bool,
                geomBuffer, binningBuffer, imageBuffer) -> torch.Tensor:
    """Test/bench introspection of the opaque state buffers (tgs_state_field)."""
    dev = geomBuffer.device
    T = ((width + 15) // 16) * ((height + 15) // 16)
    count = {"n_contrib": width * height, "final_T": width * height, "ranges": 2 * T, "point_list": R, "block_masks": R, "quad_masks": R, "means2D": 2 * P,
             "depths": P, "conic_opacity": 4 * P, "rgb": 3 * P, "tiles_touched": P, "tile_order": T, "stamps": 8 * T}[name]
    out = torch.empty((count,), dtype=_FIELD_DTYPES[name], device=dev)
    with torch.cuda.device(dev):
        r = _lib.tgs_state_field(torch.cuda.current_stream(dev).cuda_stream, name.encode(), P, width, height, int(R),
                                 int(has_sh), int(has_scale_rot), geomBuffer.data_ptr(), binningBuffer.data_ptr(),
                                 imageBuffer.data_ptr(), out.data_ptr(), out.numel() * out.element_size())
    if r < 0:
        raise _err(int(r))
    return out


# The reference's three exports (ext.cpp:15-19): the compiled module's functions, positional signatures of rasterize_points.h:18-67
# (+ the keyword extensions documented in csrc/tgs_torch_ext.cpp: r_capacity / r_guess of the forward; _with_conic, need_colors / need_cov3D and the
# upstream gradients grad_out_alpha / grad_out_depth / grad_out_features + features / grad_out_median + median_pos of the backward, which
# rasterize_gaussians_backward_accumulate above hands to the same compiled backward).
rasterize_gaussians = _ext.rasterize_gaussians
rasterize_gaussians_backward = _ext.rasterize_gaussians_backward
mark_visible = _ext.mark_visible
alpha_from_state = _ext.alpha_from_state       # (imageBuffer, H, W) -> the frame's accumulated alpha [1,H,W] = 1 - final_T (tgs_alpha; an extension)
# (geomBuffer, binningBuffer, imageBuffer, P, H, W, R) -> the frame's expected depth [1,H,W] = sum_i T_i alpha_i z_i (tgs_depth; an extension)
depth_from_state = _ext.depth_from_state
# (geomBuffer, binningBuffer, imageBuffer, features[P,C], P, H, W, R) -> the frame's feature map [C,H,W] = sum_i T_i alpha_i features[i, :]
# (tgs_features; an extension, 1 <= C <= 16)
features_from_state = _ext.features_from_state
# (geomBuffer, binningBuffer, imageBuffer, P, H, W, R) -> (median_depth[1,H,W] f32, median_index[1,H,W] i32, median_pos[1,H,W] i32): z and Gaussian
# index of the first blended pair after which T < 0.5 (0 / -1 where there is none) and its 1-based list position, which the backward's
# grad_out_median / median_pos keywords take (tgs_median; an extension)
median_from_state = _ext.median_from_state
FEATURE_MAX_CHANNELS = 16      # TGS_FEATURE_MAX_CHANNELS
