"""CPU: alpha and depth in the whole-batch path (tgs_view_extras_t beside the frozen tgs_view_t) at the C ABI and at the Python surface --
no device needed.  The GPU side is tests/test_gpu_batch_extras.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import pytest

from tests.test_depth_abi import lib_path
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_outputs_views", "tgs_backward_render_views_extras_opt", "tgs_backward_batch_depth_range", "tgs_sizeof_view_extras")
INVALID = -1


class ViewT(ctypes.Structure):
    """tgs_view_t as the header declares it (written out here: the test must not depend on the binding it checks)"""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("tan_fovx", ctypes.c_float), ("tan_fovy", ctypes.c_float),
                ("viewmatrix", ctypes.c_void_p), ("projmatrix", ctypes.c_void_p), ("campos", ctypes.c_void_p), ("radii", ctypes.c_void_p),
                ("geom_buffer", ctypes.c_void_p), ("binning_buffer", ctypes.c_void_p), ("img_buffer", ctypes.c_void_p), ("R", ctypes.c_int64),
                ("dL_dmean2D", ctypes.c_void_p), ("dL_dcolor", ctypes.c_void_p), ("background", ctypes.c_void_p), ("out_color", ctypes.c_void_p),
                ("radii_out", ctypes.c_void_p), ("dL_dpix", ctypes.c_void_p), ("geom_bytes", ctypes.c_size_t), ("binning_bytes", ctypes.c_size_t),
                ("img_bytes", ctypes.c_size_t), ("colors_precomp", ctypes.c_void_p), ("tile_bound", ctypes.c_int64), ("heavy_bound", ctypes.c_int64),
                ("mid_bound", ctypes.c_int64), ("host_meta", ctypes.c_void_p)]


class ExtrasT(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("out_alpha", ctypes.c_void_p), ("out_depth", ctypes.c_void_p), ("dL_dalpha", ctypes.c_void_p),
                ("dL_ddepth", ctypes.c_void_p), ("dz_scratch", ctypes.c_void_p)]


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it = ctypes.c_void_p, ctypes.c_int
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_sizeof_view_extras.restype = ctypes.c_size_t
    lib.tgs_outputs_views.restype = it
    lib.tgs_outputs_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_render_views_extras_opt.restype = it
    lib.tgs_backward_render_views_extras_opt.argtypes = [vp, vp, it, it, it, vp, vp]
    lib.tgs_backward_batch_depth_range.restype = it
    lib.tgs_backward_batch_depth_range.argtypes = [vp, it, it, vp, vp, vp, it, it]
    return lib


def test_header_declares_and_library_exports_the_batch_extras_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert "tgs_view_extras_t" in src and int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    # alpha and depth are part of the whole-batch path now, feature channels are not -- and the header says both
    assert "Not part of the whole-batch path" not in text
    assert "NOT part of the whole-batch path" in text and "Part of the whole-batch path" in text
    assert "tgs_set_render_streams" in text[text.index("int tgs_outputs_views") - 1500:text.index("int tgs_outputs_views")]      # the stream rule is written down
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


def test_the_frozen_sizes_stay_and_the_mirror_matches():
    lib = _lib()
    lib.tgs_abi_version.restype = ctypes.c_int
    lib.tgs_sizeof_view.restype = lib.tgs_sizeof_options.restype = ctypes.c_size_t
    assert lib.tgs_abi_version() == 3 and lib.tgs_sizeof_view() == 192 and lib.tgs_sizeof_options() == 56
    assert ctypes.sizeof(ViewT) == 192
    assert lib.tgs_sizeof_view_extras() == ctypes.sizeof(ExtrasT) == 48
    from diff_gaussian_rasterization import _C
    assert ctypes.sizeof(_C._ViewExtrasT) == lib.tgs_sizeof_view_extras()
    assert [n for n, _ in _C._ViewExtrasT._fields_] == [n for n, _ in ExtrasT._fields_]
    arr = _C.ViewExtrasArray(3)
    assert len(arr) == 3 and all(x.struct_size == 48 and x.out_alpha is None and x.dz_scratch is None for x in arr)
    # tgs_state_sizes is unchanged: the dz scratch is the caller's, not a part of the binning buffer
    sizes = (ctypes.c_size_t * 3)()
    lib.tgs_state_sizes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    lib.tgs_state_sizes.restype = None
    lib.tgs_state_sizes(1000, 200, 120, 1, 1, 5000, sizes)
    R, end = 5000, 0
    for b in (8, 4, 16, 16, 8, 4, 8, 48):
        end = ((end + 255) & ~255) + R * b
    assert sizes[1] == end + 256


def _views(n=2):
    some = 4096                                 # never dereferenced: every call below must fail (or return) in the argument checks
    arr = (ViewT * n)()
    for a in arr:
        a.width, a.height, a.R = 64, 48, 5
        for f in ("viewmatrix", "projmatrix", "campos", "radii", "geom_buffer", "binning_buffer", "img_buffer", "dL_dmean2D", "background", "dL_dpix"):
            setattr(a, f, some)
    return arr


def _extras(n=2, struct_size=None, **fields):
    arr = (ExtrasT * n)()
    for x in arr:
        x.struct_size = ctypes.sizeof(ExtrasT) if struct_size is None else struct_size
        for k, v in fields.items():
            setattr(x, k, v)
    return arr


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some = 4096
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    streams = (ctypes.c_void_p * 2)(None, None)
    views = _views()
    good = _extras(out_alpha=some, out_depth=some, dL_dalpha=some, dL_ddepth=some, dz_scratch=some)
    no_dz = _extras(dL_ddepth=some)
    small = _extras(struct_size=8, out_alpha=some)                           # smaller than the first pointer field ends (offset 8 + 8)
    calls = {
        "tgs_outputs_views": lambda P=10, n=2, v=views, x=good, s=streams, ns=2: lib.tgs_outputs_views(s, ns, P, n, v, x),
        "tgs_backward_render_views_extras_opt": lambda P=10, n=2, v=views, x=good, s=streams, ns=2: lib.tgs_backward_render_views_extras_opt(None, s, ns, P, n, v, x),
        "tgs_backward_batch_depth_range": lambda P=10, n=2, v=views, x=good, s=None, ns=1: lib.tgs_backward_batch_depth_range(None, P, n, v, x, some, 0, P),
    }
    for name, call in calls.items():
        cases = [dict(P=-1), dict(n=-1), dict(v=None), dict(x=no_dz), dict(x=small)]
        if name != "tgs_backward_batch_depth_range":
            cases += [dict(ns=0), dict(ns=-2), dict(s=None)]
        for kw in cases:
            assert call(**kw) == INVALID and name in msg(), (name, kw, msg())
        assert call(x=no_dz) == INVALID and "dz_scratch" in msg()
        assert call(x=small) == INVALID and "struct_size" in msg()
    # the Gaussian range follows the rule of tgs_backward_batch_range
    assert lib.tgs_backward_batch_depth_range(None, 1000, 2, views, good, some, 100, 256) == INVALID and "tgs_backward_batch_depth_range" in msg()
    assert lib.tgs_backward_batch_depth_range(None, 1000, 2, views, good, some, 256, 1000) == INVALID
    assert lib.tgs_backward_batch_depth_range(None, 1000, 2, views, good, None, 0, 1000) == INVALID        # a view has dL_ddepth but there is no dL_dmean3D


def test_nothing_asked_is_a_no_op():
    """no views, no extras, or no pointer set in any view: nothing is launched (the calls return before any stream is used)"""
    lib = _lib()
    streams = (ctypes.c_void_p * 1)(None)
    views, none = _views(), _extras()
    assert lib.tgs_outputs_views(streams, 1, 10, 0, None, None) == 0
    assert lib.tgs_outputs_views(streams, 1, 10, 2, views, None) == 0
    assert lib.tgs_outputs_views(streams, 1, 10, 2, views, none) == 0
    assert lib.tgs_backward_render_views_extras_opt(None, streams, 1, 0, 2, views, none) == 0              # an empty model
    assert lib.tgs_backward_batch_depth_range(None, 10, 2, views, None, None, 0, 10) == 0
    assert lib.tgs_backward_batch_depth_range(None, 10, 2, views, none, None, 0, 10) == 0                  # no view has dL_ddepth
    assert lib.tgs_backward_batch_depth_range(None, 10, 0, None, None, None, 0, 10) == 0
    assert lib.tgs_backward_batch_depth_range(None, 0, 2, views, none, None, 0, 0) == 0


def test_python_surface_without_a_device():
    from diff_gaussian_rasterization import _C
    from youreditableavatar_amd import multiview as mv
    p = inspect.signature(mv.SyncFreeBatch.run_views).parameters
    names = list(p)
    assert p["return_alpha"].default is False and p["return_depth"].default is False and names.index("return_alpha") < names.index("return_depth")
    assert names.index("on_chunk") < names.index("return_alpha")               # appended: positional callers keep their meaning
    for fn in (_C.ViewExtrasArray, _C.outputs_views, _C.backward_render_views_extras, _C.backward_batch_depth_raw):
        assert callable(fn)
    q = inspect.signature(_C.rasterize_gaussians_backward_accumulate).parameters
    for k in ("grad_out_alpha", "grad_out_depth"):
        assert q[k].kind is inspect.Parameter.KEYWORD_ONLY and q[k].default is None
    doc = mv.SyncFreeBatch.run_views.__doc__
    assert "return_alpha" in doc and "rasterize_accumulate" in doc[doc.index("return_alpha"):]        # what is not extended is said there


def test_the_upstream_tuple_check():
    import torch
    from youreditableavatar_amd.multiview import _upstream_extras_checked as check
    H, W, V = 6, 10, 3
    c = types.SimpleNamespace(H=H, W=W, V=V)
    f = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    both = ["alpha", "depth"]
    # accepted: every shape the docstring names, None for a map that took no part, non-contiguous input made contiguous
    dL, (gA, gD) = check((f(V, 3, H, W), f(V, 1, H, W), f(1, H, W)), c, both, per_view=False, require_gpu=False)
    assert tuple(gA.shape) == (V, 1, H, W) and tuple(gD.shape) == (1, H, W)
    dL, (gA, gD) = check([f(3, H, W), None, f(1, H, W)], c, both, per_view=True, require_gpu=False)
    assert gA is None and tuple(dL.shape) == (3, H, W)
    dL, (gD,) = check((f(3, H, W), f(1, W, H).transpose(1, 2)), c, ["depth"], per_view=True, require_gpu=False)
    assert gD.is_contiguous() and tuple(gD.shape) == (1, H, W)
    bad = [
        (f(V, 3, H, W), both, False),                                        # a bare tensor where a tuple is due
        ((f(V, 3, H, W), f(1, H, W)), both, False),                          # wrong arity
        ((f(V, 3, H, W), None, None, None), both, False),
        ((f(V, 3, H, W), f(3, H, W), None), both, False),                    # [3,H,W] where [1,H,W] is due
        ((f(3, H, W), f(V, 1, H, W)), ["alpha"], True),                      # the view callable returns one view's gradient
        ((f(V, 3, H, W), f(1, H, W, dt=torch.float64), None), both, False),  # float64
        ((f(V, 3, H, W), None, f(H, W)), both, False),
        ((None, f(1, H, W), None), both, False),                             # the colour gradient stays required
        ((f(V, 3, H, W, dt=torch.float64), None, None), both, False),
        ((f(V, 3, H, W), "x", None), both, False),
    ]
    for ret, names, per_view in bad:
        with pytest.raises(RuntimeError, match="upstream"):
            check(ret, c, names, per_view=per_view, require_gpu=False)
    # on the real path the gradients must be on the device
    with pytest.raises(RuntimeError, match="GPU"):
        check((f(3, H, W), f(1, H, W)), c, ["alpha"], per_view=True)
