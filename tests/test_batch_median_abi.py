"""CPU: the median of a batch's views (tgs_view_median_t, the fourth per-view array), the surface votes and their Python surface -- no device
needed -- and the yardstick the GPU tests of tests/test_gpu_batch_median.py measure against.

The yardstick is the one of tests/test_median_abi.py (median_walk: a NumPy walk of the oracle's own lists, in float32 on the fp32 oracle's
state and in float64 on the fp64 oracle's; a pixel is AMBIGUOUS if the two walks disagree on its index or a blended pair leaves T within
0.5e-4 of one half), taken per view of the six scenes of tests/test_gpu_batch_extras.py (SCENES + [PRECOMP], 176 x 112, make_scene)."""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import util
from tests.test_batch_extras_abi import ViewT, _views
from tests.test_depth_abi import lib_path
from tests.test_median_abi import AMBIGUOUS_CAP, median_walk
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_sizeof_view_median", "tgs_median_views", "tgs_backward_median_views", "tgs_backward_batch_median_range", "tgs_surface_votes")
INVALID = -1
RUN_VIEWS_PARAMETERS = ["self", "settings", "means3D", "opacities", "shs", "scales", "rotations", "upstream_batch", "accumulate", "colors_precomp",
                        "upstream_view", "grad_chunks", "on_chunk", "return_alpha", "return_depth", "features"]


class MedianT(ctypes.Structure):
    """tgs_view_median_t as the header declares it (written out here: the test must not depend on the binding it checks)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("out_depth", ctypes.c_void_p), ("out_index", ctypes.c_void_p), ("out_pos", ctypes.c_void_p),
                ("dL_dmedian_depth", ctypes.c_void_p), ("dz_scratch", ctypes.c_void_p)]


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it = ctypes.c_void_p, ctypes.c_int
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_sizeof_view_median.restype = ctypes.c_size_t
    lib.tgs_median_views.restype = it
    lib.tgs_median_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_median_views.restype = it
    lib.tgs_backward_median_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_batch_median_range.restype = it
    lib.tgs_backward_batch_median_range.argtypes = [vp, it, it, vp, vp, vp, it, it]
    lib.tgs_surface_votes.restype = it
    lib.tgs_surface_votes.argtypes = [vp, it, ctypes.c_int64, vp, vp, vp, vp]
    return lib


# ---- the yardstick of the batch scenes ----
def batch_scenes():
    from tests import test_gpu_batch_extras as E
    return E.SCENES + [E.PRECOMP]


def scene_id(case):
    return f"P{case[0]}-V{case[1]}-D{case[2]}-M{case[3]}"


@functools.lru_cache(maxsize=None)
def yardstick(P, V, D, M, seed, scale_mult):
    """-> the scene of tests/test_gpu_batch_extras.py (cloud, cameras, colour upstreams) and per view the fp32 and fp64 walks, the ambiguous
    pixels and the fp32 oracle's depths / radii (computed once per scene, read-only)"""
    from tests.test_gpu_batch_extras import H, W
    from tests.test_gpu_batch_backward import make_scene
    cloud, cams, dLs = make_scene(P, V, D, M, False, seed, scale_mult, False)
    views = []
    for cam in cams:
        inp = util.scene_input(cloud, cam, "sh" if M else "precomp")
        y = {}
        for variant, dtype in (("f32", np.float32), ("f64", np.float64)):
            o = util.oracle_run(inp, None, variant=variant)
            y[variant] = median_walk(o, H, W, dtype)
            if variant == "f32":
                y["depths"], y["radii"] = np.asarray(o["depths"]).reshape(-1), np.asarray(o["radii"])
        y["ambiguous"] = (y["f32"]["index"] != y["f64"]["index"]) | y["f32"]["near"]
        y["index"], y["ok"] = y["f32"]["index"], ~y["ambiguous"]
        for a in (y["ambiguous"], y["index"], y["ok"], y["depths"]):
            a.setflags(write=False)
        views.append(y)
    return dict(cloud=cloud, cams=cams, dLs=dLs, views=views, P=P, V=V, D=D, M=M, H=H, W=W)


@pytest.mark.parametrize("case", batch_scenes(), ids=scene_id)
def test_the_yardstick_of_the_batch_scenes(case):
    """A guard on the reference, not on the code under test: per view at most AMBIGUOUS_CAP of the pixels are ambiguous and the two walks
    agree on the others; every scene but P1-V1 has median pixels in every view, P1-V1 has none (the "no surface anywhere" case)."""
    y = yardstick(*case[:6])
    N = y["H"] * y["W"]
    for v, w in enumerate(y["views"]):
        amb, has = int(w["ambiguous"].sum()), int((w["index"] >= 0).sum())
        print(f"{scene_id(case)} view {v}: {amb} ambiguous pixels of {N} ({100.0 * amb / N:.3f} %), {has} with a median entry")
        assert amb <= AMBIGUOUS_CAP * N
        assert np.array_equal(w["f32"]["index"][w["ok"]], w["f64"]["index"][w["ok"]])
        assert np.all((w["radii"] > 0)[w["index"][w["index"] >= 0]]), "a culled Gaussian cannot be a median entry"
        assert (has == 0) if case[0] == 1 else (has > 1000)


# ---- the C ABI ----
def test_header_declares_and_library_exports_the_batch_median_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert "tgs_view_median_t" in src and int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    assert "the *_views entry points have no median" not in text                                   # the old sentence is gone
    assert "tgs_set_render_streams" in text[text.index("int tgs_outputs_views") - 1500:text.index("int tgs_outputs_views")]
    assert "written above tgs_outputs_views" in text[text.index("int tgs_median_views") - 1200:text.index("int tgs_median_views")]      # the stream rule is referred to
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


def test_the_frozen_sizes_stay_and_the_mirror_matches():
    lib = _lib()
    lib.tgs_abi_version.restype = ctypes.c_int
    for f in ("tgs_sizeof_view", "tgs_sizeof_options", "tgs_sizeof_view_extras", "tgs_sizeof_view_features"):
        getattr(lib, f).restype = ctypes.c_size_t
    assert lib.tgs_abi_version() == 3
    assert (lib.tgs_sizeof_view(), lib.tgs_sizeof_view_extras(), lib.tgs_sizeof_view_features(), lib.tgs_sizeof_options()) == (192, 48, 40, 56)
    assert ctypes.sizeof(ViewT) == 192
    from diff_gaussian_rasterization import _C
    assert lib.tgs_sizeof_view_median() == ctypes.sizeof(MedianT) == ctypes.sizeof(_C._ViewMedianT) == 48
    assert [n for n, _ in _C._ViewMedianT._fields_] == [n for n, _ in MedianT._fields_] == \
        ["struct_size", "out_depth", "out_index", "out_pos", "dL_dmedian_depth", "dz_scratch"]
    assert [MedianT.out_depth.offset, MedianT.out_index.offset, MedianT.out_pos.offset, MedianT.dL_dmedian_depth.offset, MedianT.dz_scratch.offset] == [8, 16, 24, 32, 40]
    arr = _C.ViewMedianArray(3)
    assert len(arr) == 3 and all(x.struct_size == 48 and x.out_depth is None and x.out_pos is None and x.dz_scratch is None for x in arr)


def _med(n=2, struct_size=None, **fields):
    arr = (MedianT * n)()
    for x in arr:
        x.struct_size = ctypes.sizeof(MedianT) if struct_size is None else struct_size
        for k, v in fields.items():
            setattr(x, k, v)
    return arr


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some = 4096                                 # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    streams = (ctypes.c_void_p * 2)(None, None)
    views = _views()
    good = _med(out_depth=some, out_index=some, out_pos=some, dL_dmedian_depth=some, dz_scratch=some)
    partial = [_med(out_depth=some), _med(out_depth=some, out_index=some), _med(out_index=some, out_pos=some)]      # the three maps come together
    no_dz = _med(out_depth=some, out_index=some, out_pos=some, dL_dmedian_depth=some)
    no_pos = _med(dL_dmedian_depth=some, dz_scratch=some)
    small = _med(struct_size=8, out_depth=some)                              # smaller than the first pointer field ends (offset 8 + 8)
    uneven = _med(out_depth=some, out_index=some, out_pos=some)
    uneven[1].struct_size = 40                                               # an element whose struct_size differs from the array's
    calls = {
        "tgs_median_views": lambda P=10, n=2, v=views, x=good, s=streams, ns=2: lib.tgs_median_views(s, ns, P, n, v, x),
        "tgs_backward_median_views": lambda P=10, n=2, v=views, x=good, s=streams, ns=2: lib.tgs_backward_median_views(s, ns, P, n, v, x),
        "tgs_backward_batch_median_range": lambda P=10, n=2, v=views, x=good, s=None, ns=1: lib.tgs_backward_batch_median_range(None, P, n, v, x, some, 0, P),
    }
    for name, call in calls.items():
        cases = [dict(P=-1), dict(n=-1), dict(v=None), dict(x=no_dz), dict(x=no_pos), dict(x=small), dict(x=uneven)] + [dict(x=p) for p in partial]
        if name != "tgs_backward_batch_median_range":
            cases += [dict(ns=0), dict(ns=-2), dict(s=None)]
        for kw in cases:
            assert call(**kw) == INVALID and name in msg(), (name, kw, msg())
        assert call(x=no_dz) == INVALID and "dz_scratch" in msg()
        assert call(x=no_pos) == INVALID and "out_pos" in msg()
        assert call(x=small) == INVALID and "struct_size" in msg()
        assert call(x=partial[0]) == INVALID and "come together" in msg()
    # the Gaussian range follows the rule of tgs_backward_batch_range
    assert lib.tgs_backward_batch_median_range(None, 1000, 2, views, good, some, 100, 256) == INVALID and "tgs_backward_batch_median_range" in msg()
    assert lib.tgs_backward_batch_median_range(None, 1000, 2, views, good, some, 256, 1000) == INVALID
    assert lib.tgs_backward_batch_median_range(None, 1000, 2, views, good, None, 0, 1000) == INVALID       # a view has a gradient but there is no dL_dmean3D
    # the first view's frame is not there (the first: nothing may be enqueued in front of the error)
    broken = _views()
    broken[0].binning_buffer = None
    assert lib.tgs_backward_median_views(streams, 2, 10, 2, broken, good) == INVALID and "tgs_backward_median_views" in msg() and "view 0" in msg()
    assert lib.tgs_median_views(streams, 2, 10, 2, broken, good) == INVALID and "tgs_median_views" in msg() and "view 0" in msg()
    broken = _views()
    broken[0].width = 0
    assert lib.tgs_backward_median_views(streams, 2, 10, 2, broken, good) == INVALID and "view 0" in msg()
    assert lib.tgs_median_views(streams, 2, 10, 2, broken, good) == INVALID and "tgs_median_views" in msg() and "view 0" in msg()
    # the votes
    votes = lambda P=10, n=100, index=some, mask=some, seen=some, hits=some: lib.tgs_surface_votes(None, P, n, index, mask, seen, hits)
    for kw in (dict(P=-1), dict(n=-1), dict(index=None), dict(seen=None), dict(hits=None), dict(seen=None, mask=None, hits=None), dict(n=1 << 40)):
        assert votes(**kw) == INVALID and "tgs_surface_votes" in msg(), (kw, msg())


def test_nothing_asked_is_a_no_op():
    """no views, no array, no pointer set in any view, an empty model, frames without instances: nothing is launched (the calls return
    before any stream is used)"""
    lib = _lib()
    some = 4096
    streams = (ctypes.c_void_p * 1)(None)
    views, none = _views(), _med()
    grads = _med(out_depth=some, out_index=some, out_pos=some, dL_dmedian_depth=some, dz_scratch=some)
    empty = _views()
    for a in empty:
        a.R = 0
    for f in (lib.tgs_median_views, lib.tgs_backward_median_views):
        assert f(streams, 1, 10, 0, None, None) == 0
        assert f(streams, 1, 10, 2, views, None) == 0
        assert f(streams, 1, 10, 2, views, none) == 0
    assert lib.tgs_backward_median_views(streams, 1, 0, 2, views, grads) == 0                              # an empty model
    assert lib.tgs_backward_median_views(streams, 1, 10, 2, empty, grads) == 0                             # R == 0 in every view
    assert lib.tgs_backward_batch_median_range(None, 10, 2, views, None, None, 0, 10) == 0
    assert lib.tgs_backward_batch_median_range(None, 10, 2, views, none, None, 0, 10) == 0                 # no view has a gradient
    assert lib.tgs_backward_batch_median_range(None, 10, 0, None, None, None, 0, 10) == 0
    assert lib.tgs_backward_batch_median_range(None, 0, 2, views, none, None, 0, 0) == 0
    assert lib.tgs_backward_batch_median_range(None, 10, 2, views, grads, some, 0, 0) == 0                 # an empty range
    assert lib.tgs_backward_batch_median_range(None, 10, 2, empty, grads, some, 0, 10) == 0                # R == 0 in every view
    assert lib.tgs_surface_votes(None, 0, 100, None, None, None, None) == 0
    assert lib.tgs_surface_votes(None, 10, 0, None, None, None, None) == 0


# ---- binding and public API ----
def test_python_surface_without_a_device():
    import torch
    from diff_gaussian_rasterization import _C
    from youreditableavatar_amd import multiview as mv
    assert list(inspect.signature(mv.SyncFreeBatch.run_views).parameters) == RUN_VIEWS_PARAMETERS
    for fn in (_C.ViewMedianArray, _C.median_views, _C.backward_median_views, _C.backward_batch_median_raw, _C.surface_votes, mv.surface_votes,
               mv.SyncFreeBatch.median_views, mv.SyncFreeBatch.backward_median_views):
        assert callable(fn)
    assert list(inspect.signature(_C.median_views).parameters) == ["stream_handles", "P", "views", "med", "n_views"]
    assert list(inspect.signature(_C.backward_median_views).parameters) == ["stream_handles", "P", "views", "med", "n_views"]
    assert list(inspect.signature(_C.backward_batch_median_raw).parameters) == ["stream", "P", "views", "med", "n_views", "dL_dmean3D", "first", "count"]
    q = inspect.signature(_C.surface_votes).parameters
    assert list(q) == ["index", "P", "mask", "out"] and q["mask"].default is None and q["out"].default is None
    q = inspect.signature(mv.surface_votes).parameters
    assert list(q) == ["median_index", "P", "masks", "out"] and q["masks"].default is None and q["out"].default is None
    # median_views on a fresh object raises; the docstrings say what is undefined and what raises
    with pytest.raises(RuntimeError, match="run_views"):
        mv.SyncFreeBatch().median_views()
    with pytest.raises(RuntimeError, match="median_views"):
        mv.SyncFreeBatch().backward_median_views(torch.zeros(1, 4, 4))
    assert "undefined" in mv.SyncFreeBatch.median_views.__doc__ and "on_chunk" in mv.SyncFreeBatch.backward_median_views.__doc__
    assert "median_views()" in mv.SyncFreeBatch.run_views.__doc__
    # the votes reject what is not an index map on a device before anything is launched
    idx = torch.zeros((2, 1, 4, 5), dtype=torch.int32)
    for bad in (idx.long(), idx.float(), idx[:, 0], idx.expand(2, 3, 4, 5)):
        with pytest.raises(RuntimeError, match="median_index"):
            mv.surface_votes(bad, 7)
    for bad in (torch.zeros((2, 1, 4, 5)), torch.zeros((1, 4, 5), dtype=torch.bool), "x"):
        with pytest.raises(RuntimeError, match="masks"):
            mv.surface_votes(idx, 7, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        mv.surface_votes(idx, 7)


def _stub_batch(V, H, W, chunked=False):
    """a SyncFreeBatch that looks as if run_views and median_views had run: the argument checks of backward_median_views come first"""
    from youreditableavatar_amd import multiview as mv
    b = mv.SyncFreeBatch()
    b._last = dict(c=types.SimpleNamespace(V=V, H=H, W=W), pool=None, sync=[], chunked=chunked, median=True)
    return b


def test_backward_median_views_checks_its_argument():
    import torch
    from youreditableavatar_amd.multiview import _median_upstreams_checked as check
    H, W, V = 6, 10, 3
    c = types.SimpleNamespace(H=H, W=W, V=V)
    f = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    # accepted: every shape the docstring names, None for a view that takes no part, non-contiguous input made contiguous
    gs = check(f(V, 1, H, W), c, require_gpu=False)
    assert len(gs) == V and all(tuple(g.shape) == (1, H, W) for g in gs)
    shared = f(1, H, W)
    assert all(g is shared for g in check(shared, c, require_gpu=False))
    gs = check([f(1, H, W), None, f(1, W, H).transpose(1, 2)], c, require_gpu=False)
    assert gs[1] is None and gs[2].is_contiguous() and tuple(gs[2].shape) == (1, H, W)
    assert check((None, None, None), c, require_gpu=False) == [None, None, None]
    bad = [f(V, H, W), f(V, 3, H, W), f(H, W), f(V + 1, 1, H, W), f(V, 1, H, W, dt=torch.float64), f(1, H, W, dt=torch.int32),
           [f(1, H, W), None], [f(1, H, W)] * (V + 1), [f(1, H, W), f(H, W), None], [f(1, H, W), f(1, H, W, dt=torch.float64), None],
           [f(1, H, W), "x", None], [f(V, 1, H, W), None, None], None, "x"]
    for dL in bad:
        with pytest.raises(RuntimeError, match="backward_median_views"):
            check(dL, c, require_gpu=False)
    # on the real path the gradients must be on the device: through the method, which checks before it touches one
    for dL in (f(V, 1, H, W), [f(1, H, W), None, None]):
        with pytest.raises(RuntimeError, match="GPU"):
            _stub_batch(V, H, W).backward_median_views(dL)
    with pytest.raises(RuntimeError, match="backward_median_views"):
        _stub_batch(V, H, W).backward_median_views(f(V, 3, H, W))
    # after a call with on_chunk the ranges were handed out as final
    with pytest.raises(RuntimeError, match="on_chunk"):
        _stub_batch(V, H, W, chunked=True).backward_median_views(f(V, 1, H, W))


def test_the_docs_carry_the_mask_lifting_recipe():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4i" in text or "### 4i" in text
    sec = text[text.index("4i"):]
    for what in ("median_views", "backward_median_views", "surface_votes", "seen", "hits", "hits / seen", "_face_indices[", "read-back"):
        assert what in sec, what
    assert "not part of the whole-batch path" not in text[text.index("4h"):text.index("4i")].replace("\n", " ")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "median_views" in readme and "surface_votes" in readme
