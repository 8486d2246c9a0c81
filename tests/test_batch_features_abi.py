"""CPU: feature channels in the whole-batch path (tgs_view_features_t, a third array beside tgs_view_t and tgs_view_extras_t) at the C ABI and
at the Python surface -- no device needed.  The GPU side is tests/test_gpu_batch_features.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import pytest

from tests.test_batch_extras_abi import ExtrasT, ViewT, _extras, _views
from tests.test_depth_abi import lib_path
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_features_views", "tgs_backward_render_views_features_opt", "tgs_backward_batch_features_range", "tgs_sizeof_view_features")
INVALID = -1


class FeaturesT(ctypes.Structure):
    """tgs_view_features_t as the header declares it (written out here: the test must not depend on the binding it checks)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("features", ctypes.c_void_p), ("out_features", ctypes.c_void_p),
                ("dL_dfeature_map", ctypes.c_void_p), ("feature_scratch", ctypes.c_void_p)]


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it = ctypes.c_void_p, ctypes.c_int
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_sizeof_view_features.restype = ctypes.c_size_t
    lib.tgs_features_views.restype = it
    lib.tgs_features_views.argtypes = [vp, it, it, it, vp, vp]
    lib.tgs_backward_render_views_features_opt.restype = it
    lib.tgs_backward_render_views_features_opt.argtypes = [vp, vp, it, it, it, vp, vp, vp]
    lib.tgs_backward_batch_features_range.restype = it
    lib.tgs_backward_batch_features_range.argtypes = [vp, it, it, vp, vp, vp, it, it, it]
    return lib


def _feats(n=2, struct_size=None, C=5, **fields):
    arr = (FeaturesT * n)()
    for x in arr:
        x.struct_size = ctypes.sizeof(FeaturesT) if struct_size is None else struct_size
        x.C = C
        for k, v in fields.items():
            setattr(x, k, v)
    return arr


def test_header_declares_and_library_exports_the_batch_feature_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert "tgs_view_features_t" in src and int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    # the struct as the issue words it, field by field and in that order
    body = re.search(r"typedef struct \{([^}]*)\} tgs_view_features_t;", src).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in FeaturesT._fields_]
    # features are part of the whole-batch path now, and the header says what still is not, in these words
    assert "Not part of the whole-batch path" not in text
    assert "NOT part of the whole-batch path" in text and "Part of the whole-batch path" in text
    rest = text[text.index("NOT part of the whole-batch path"):][:400]
    for what in ("median / mode depth", "more than 16 channels", "half-precision features", "tgs_backward_batch without ranges"):
        assert what in rest, what
    assert "can be appended" not in text                                      # the promise the extras descriptor did not keep is gone
    head = text[text.index("int tgs_features_views") - 1200:text.index("int tgs_features_views")]
    assert "tgs_outputs_views" in head and "tgs_set_render_streams" in head  # the stream rule: pointed to and said again
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


def test_the_frozen_sizes_stay_and_the_mirror_matches():
    lib = _lib()
    lib.tgs_abi_version.restype = ctypes.c_int
    lib.tgs_sizeof_view.restype = lib.tgs_sizeof_options.restype = lib.tgs_sizeof_view_extras.restype = ctypes.c_size_t
    assert lib.tgs_abi_version() == 3 and lib.tgs_sizeof_view() == 192 and lib.tgs_sizeof_options() == 56 and lib.tgs_sizeof_view_extras() == 48
    assert ctypes.sizeof(ViewT) == 192 and ctypes.sizeof(ExtrasT) == 48
    assert lib.tgs_sizeof_view_features() == ctypes.sizeof(FeaturesT) == 40
    assert FeaturesT.features.offset == 8 and FeaturesT.feature_scratch.offset == 32
    from diff_gaussian_rasterization import _C
    assert ctypes.sizeof(_C._ViewFeaturesT) == lib.tgs_sizeof_view_features()
    assert [(n, ctypes.sizeof(t)) for n, t in _C._ViewFeaturesT._fields_] == [(n, ctypes.sizeof(t)) for n, t in FeaturesT._fields_]
    arr = _C.ViewFeaturesArray(3)
    assert len(arr) == 3
    for x in arr:
        assert x.struct_size == 40 and x.C == 0
        assert x.features is None and x.out_features is None and x.dL_dfeature_map is None and x.feature_scratch is None
    # tgs_state_sizes is unchanged: the feature scratch is the caller's, not a part of the binning buffer
    sizes = (ctypes.c_size_t * 3)()
    lib.tgs_state_sizes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    lib.tgs_state_sizes.restype = None
    lib.tgs_state_sizes(1000, 200, 120, 1, 1, 5000, sizes)
    R, end = 5000, 0
    for b in (8, 4, 16, 16, 8, 4, 8, 48):
        end = ((end + 255) & ~255) + R * b
    assert sizes[1] == end + 256


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = 4096, 8192                    # never dereferenced: every call below must fail (or return) in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    streams = (ctypes.c_void_p * 2)(None, None)
    views = _views()
    full = dict(features=some, out_features=some, dL_dfeature_map=some, feature_scratch=some)
    good = _feats(**full)
    small = _feats(struct_size=8, **full)                                    # ends in front of the features field (offset 8 + 8)
    mixed = _feats(**full)
    mixed[1].struct_size = 32                                                # differing struct_size within an array
    no_features = _feats(out_features=some)
    no_features2 = _feats(dL_dfeature_map=some, feature_scratch=some)
    no_scratch = _feats(features=some, dL_dfeature_map=some)
    other_C = _feats(**full)
    other_C[1].C = 4
    other_F = _feats(**full)
    other_F[1].features = other
    calls = {
        "tgs_features_views": lambda P=10, n=2, v=views, f=good, s=streams, ns=2: lib.tgs_features_views(s, ns, P, n, v, f),
        "tgs_backward_render_views_features_opt":
            lambda P=10, n=2, v=views, f=good, s=streams, ns=2, x=None: lib.tgs_backward_render_views_features_opt(None, s, ns, P, n, v, x, f),
        "tgs_backward_batch_features_range":
            lambda P=10, n=2, v=views, f=good, s=None, ns=1, d=some, acc=0: lib.tgs_backward_batch_features_range(None, P, n, v, f, d, acc, 0, max(P, 0)),
    }
    for name, call in calls.items():
        cases = [dict(P=-1), dict(n=-1), dict(v=None), dict(f=small), dict(f=mixed), dict(f=_feats(C=0, **full)), dict(f=_feats(C=17, **full)),
                 dict(f=_feats(C=-3, features=some)), dict(f=_feats(C=0, out_features=some)), dict(f=other_C), dict(f=other_F), dict(f=no_features),
                 dict(f=no_features2), dict(f=no_scratch)]
        if name != "tgs_backward_batch_features_range":
            cases += [dict(ns=0), dict(ns=-2), dict(s=None)]
        for kw in cases:
            assert call(**kw) == INVALID and name in msg(), (name, kw, msg())
        assert call(f=small) == INVALID and "struct_size" in msg()
        assert call(f=mixed) == INVALID and "struct_size" in msg()
        assert call(f=_feats(C=17, **full)) == INVALID and "17" in msg()
        assert call(f=no_scratch) == INVALID and "feature_scratch" in msg()
        assert call(f=no_features) == INVALID and "without features" in msg()
        assert call(f=other_C) == INVALID and "differ" in msg()
    # the extras of the render call are checked as tgs_backward_render_views_extras_opt checks them
    assert calls["tgs_backward_render_views_features_opt"](x=_extras(dL_ddepth=some)) == INVALID and "dz_scratch" in msg()
    # the Gaussian range follows the rule of tgs_backward_batch_range
    rng = lambda first, count, d=some, f=good, P=1000: lib.tgs_backward_batch_features_range(None, P, 2, views, f, d, 0, first, count)
    assert rng(100, 256) == INVALID and "tgs_backward_batch_features_range" in msg()
    assert rng(256, 1000) == INVALID and rng(0, 300) == INVALID and rng(-256, 256) == INVALID and rng(0, -1) == INVALID
    # a view takes part but there is nowhere to put the gradient
    assert rng(0, 1000, d=None) == INVALID and "dL_dfeatures" in msg()
    assert lib.tgs_backward_batch_features_range(None, 1000, 2, views, good, None, 1, 0, 1000) == INVALID


def test_nothing_asked_is_a_no_op():
    """no views, no feats, no pointer set in any view, an empty model, or nothing to add: nothing is launched (the calls return before any
    stream is used)"""
    lib = _lib()
    some = 4096
    streams = (ctypes.c_void_p * 1)(None)
    views, none = _views(), _feats(C=0)
    only_maps = _feats(features=some, out_features=some)                     # a forward-only step: no view has a gradient of the map
    assert lib.tgs_features_views(streams, 1, 10, 0, None, None) == 0
    assert lib.tgs_features_views(streams, 1, 10, 2, views, None) == 0
    assert lib.tgs_features_views(streams, 1, 10, 2, views, none) == 0
    assert lib.tgs_features_views(streams, 1, 10, 2, views, _feats(features=some)) == 0                   # features alone ask for nothing
    assert lib.tgs_backward_render_views_features_opt(None, streams, 1, 10, 0, None, None, None) == 0
    assert lib.tgs_backward_render_views_features_opt(None, streams, 1, 0, 2, views, None, _feats(features=some, dL_dfeature_map=some, feature_scratch=some)) == 0   # an empty model
    assert lib.tgs_backward_render_views_features_opt(None, streams, 1, 0, 2, views, _extras(), none) == 0
    rng = lib.tgs_backward_batch_features_range
    assert rng(None, 10, 0, None, None, None, 0, 0, 10) == 0
    assert rng(None, 10, 2, views, None, None, 0, 0, 10) == 0
    assert rng(None, 10, 2, views, none, None, 0, 0, 10) == 0                # no pointer set: not even C is known
    assert rng(None, 10, 2, views, none, some, 0, 0, 10) == 0
    assert rng(None, 0, 2, views, only_maps, some, 0, 0, 0) == 0             # an empty model
    assert rng(None, 10, 2, views, only_maps, some, 1, 0, 10) == 0           # accumulate and no view takes part: nothing to add
    assert rng(None, 10, 2, views, only_maps, None, 1, 0, 10) == 0
    empty = _views()
    for a in empty:
        a.R = 0                                                              # gradients, but no view has instances: the same
    assert rng(None, 10, 2, empty, _feats(features=some, dL_dfeature_map=some, feature_scratch=some), some, 1, 0, 10) == 0


def test_python_surface_without_a_device():
    from diff_gaussian_rasterization import _C
    from youreditableavatar_amd import multiview as mv
    p = inspect.signature(mv.SyncFreeBatch.run_views).parameters
    names = list(p)
    assert names[-1] == "features" and p["features"].default is None and names[-2] == "return_depth"       # appended: positional callers keep their meaning
    assert p["return_alpha"].default is False and p["return_depth"].default is False
    for fn in (_C.ViewFeaturesArray, _C.features_views, _C.backward_render_views_features, _C.backward_batch_features_raw):
        assert callable(fn)
    assert list(inspect.signature(_C.features_views).parameters) == ["stream_handles", "P", "views", "feats", "n_views"]
    assert list(inspect.signature(_C.backward_render_views_features).parameters) == ["stream_handles", "P", "views", "extras", "feats", "n_views", "opt"]
    q = inspect.signature(_C.backward_batch_features_raw).parameters
    assert list(q) == ["stream", "P", "views", "feats", "n_views", "dL_dfeatures", "accumulate", "first", "count"] and q["first"].default == 0 and q["count"].default is None
    q = inspect.signature(_C.rasterize_gaussians_backward_accumulate).parameters
    for k in ("grad_out_alpha", "grad_out_depth", "grad_out_features", "features"):
        assert q[k].kind is inspect.Parameter.KEYWORD_ONLY and q[k].default is None
    doc = mv.SyncFreeBatch.run_views.__doc__
    assert "return_alpha" in doc and "rasterize_accumulate" in doc[doc.index("return_alpha"):]        # what is not extended is said there
    assert "features" in doc and "rasterize_accumulate" in doc[doc.index("``features``"):]
    assert "feature channels are not part of this path" not in doc
    assert "* 4 bytes" in doc                                                                         # the size of the scratch is stated


def test_the_upstream_tuple_check_with_a_feature_map():
    import torch
    from youreditableavatar_amd.multiview import _upstream_extras_checked as check
    H, W, V, C = 6, 10, 3, 5
    c = types.SimpleNamespace(H=H, W=W, V=V)
    f = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    ch = {"features": C}
    all3 = ["alpha", "depth", "features"]
    # accepted: [V,C,H,W], [C,H,W] and None; alpha / depth keep one channel beside it
    dL, (gF,) = check((f(V, 3, H, W), f(V, C, H, W)), c, ["features"], per_view=False, require_gpu=False, channels=ch)
    assert tuple(gF.shape) == (V, C, H, W)
    dL, (gA, gD, gF) = check((f(V, 3, H, W), f(1, H, W), None, f(C, H, W)), c, all3, per_view=False, require_gpu=False, channels=ch)
    assert tuple(gA.shape) == (1, H, W) and gD is None and tuple(gF.shape) == (C, H, W)
    dL, (gF,) = check([f(3, H, W), None], c, ["features"], per_view=True, require_gpu=False, channels=ch)
    assert gF is None
    dL, (gF,) = check((f(3, H, W), f(C, W, H).transpose(1, 2)), c, ["features"], per_view=True, require_gpu=False, channels=ch)
    assert gF.is_contiguous() and tuple(gF.shape) == (C, H, W)
    dL, (gF,) = check((f(3, H, W), f(1, H, W)), c, ["features"], per_view=True, require_gpu=False, channels={"features": 1})     # C = 1 is [1,H,W]
    assert tuple(gF.shape) == (1, H, W)
    bad = [
        ((f(V, 3, H, W), f(1, H, W)), ["features"], False),                  # [1,H,W] where [C,H,W] is due, C != 1
        ((f(V, 3, H, W), f(V, 1, H, W)), ["features"], False),
        ((f(V, 3, H, W), f(C + 1, H, W)), ["features"], False),
        ((f(V, 3, H, W), f(C, H, W), None, f(C, H, W)), all3, False),        # the channel count belongs to the name: alpha stays [1,H,W]
        ((f(V, 3, H, W), None, f(C, H, W), None), all3, False),
        ((f(3, H, W), f(V, C, H, W)), ["features"], True),                   # the view callable returns one view's gradient
        ((f(V, 3, H, W), f(C, H, W, dt=torch.float64)), ["features"], False),
        ((f(V, 3, H, W),), ["features"], False),                             # wrong arity
        ((f(V, 3, H, W), None, None), ["features"], False),
        (f(V, 3, H, W), ["features"], False),                                # a bare tensor where a tuple is due
        ((f(V, 3, H, W), "x"), ["features"], False),                         # not a tensor
        ((f(V, 3, H, W), [[0.0]]), ["features"], False),
        ((None, f(C, H, W)), ["features"], False),                           # the colour gradient stays required
    ]
    for ret, names, per_view in bad:
        with pytest.raises(RuntimeError, match="upstream"):
            check(ret, c, names, per_view=per_view, require_gpu=False, channels=ch)
    with pytest.raises(RuntimeError, match="GPU"):
        check((f(3, H, W), f(C, H, W)), c, ["features"], per_view=True, channels=ch)
    # every case of the existing check behaves as before (no channels: one per name)
    from tests.test_batch_extras_abi import test_the_upstream_tuple_check
    test_the_upstream_tuple_check()


def test_the_upstream_caller_of_run_views_without_a_device():
    """multiview._Upstream, what every route of run_views asks the upstream callables through: it passes the extra maps when the call has
    any, accepts what the docstring of run_views lists, and rejects the rest with the messages of the pooled route."""
    import torch
    from youreditableavatar_amd.multiview import _Upstream
    H, W, V, C = 6, 10, 3, 5
    f = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    images, maps3 = f(V, 3, H, W), [f(V, 1, H, W), f(V, 1, H, W), f(V, C, H, W)]
    plain = types.SimpleNamespace(H=H, W=W, V=V, names=[], Cf=0)
    full = types.SimpleNamespace(H=H, W=W, V=V, names=["alpha", "depth", "features"], Cf=C)
    seen = []

    def caller(c, ret):
        def batch(*args):
            seen.append(("batch", [tuple(a.shape) for a in args]))
            return ret
        def view(v, *args):
            seen.append((v, [tuple(a.shape) for a in args]))
            return ret
        return _Upstream(c, batch, None, require_gpu=False), _Upstream(c, None, view, require_gpu=False)

    # without extra maps: a bare tensor, [V,3,H,W] or [3,H,W] from the batch callable, [3,H,W] from the view callable; made contiguous
    for ret in (f(V, 3, H, W), f(3, H, W), f(3, W, H).transpose(1, 2)):
        b, _ = caller(plain, ret)
        assert not b.per_view
        dL, extra = b.batch(images, [])
        assert dL.is_contiguous() and tuple(dL.shape) == tuple(ret.shape) and len(extra) == V and all(len(e) == 0 for e in extra)
        g, gs = b.views(images, [])(1)
        assert tuple(g.shape) == (3, H, W) and len(gs) == 0
    _, w = caller(plain, f(3, H, W))
    assert w.per_view
    g, gs = w.view(2, images, [])
    assert tuple(g.shape) == (3, H, W) and len(gs) == 0 and seen[-1] == (2, [(3, H, W)])
    g, gs = w.views(images, [])(0)
    assert tuple(g.shape) == (3, H, W) and seen[-1] == (0, [(3, H, W)])
    # with extra maps: the tuple, every extra entry [V,C,H,W], [C,H,W] or None from the batch callable, [C,H,W] or None from the view callable
    b, _ = caller(full, (f(V, 3, H, W), f(V, 1, H, W), None, f(C, H, W)))
    dL, extra = b.batch(images, maps3)
    assert seen[-1] == ("batch", [(V, 3, H, W), (V, 1, H, W), (V, 1, H, W), (V, C, H, W)])
    assert len(extra) == V and all(tuple(e[0].shape) == (1, H, W) and e[1] is None and tuple(e[2].shape) == (C, H, W) for e in extra)
    g, gs = b.views(images, maps3)(2)
    assert tuple(g.shape) == (3, H, W) and tuple(gs[0].shape) == (1, H, W) and gs[1] is None
    _, w = caller(full, (f(3, H, W), None, f(1, H, W), f(C, H, W)))
    g, gs = w.view(1, images, maps3)
    assert seen[-1] == (1, [(3, H, W), (1, H, W), (1, H, W), (C, H, W)])
    assert tuple(g.shape) == (3, H, W) and gs[0] is None and tuple(gs[1].shape) == (1, H, W) and tuple(gs[2].shape) == (C, H, W)
    # rejected, with the messages of the pooled route
    bare = "upstream must return a float32 GPU tensor [V,3,H,W] or [3,H,W]"
    tup = ("upstream must return the tuple (dL_dimages, dL_dalpha, dL_ddepth, dL_dfeatures) when run_views returns alpha and depth and features "
           "(an entry may be None, the first may not)")
    one = "upstream_view must return [3,H,W]"
    bad = [
        (plain, f(V, 3, H, W, dt=torch.float64), bare, bare),                                    # float64
        (plain, f(V, 3, H, W + 1), bare, bare),                                                  # a wrong shape
        (plain, (f(V, 3, H, W),), bare, bare),                                                   # a tuple where a bare tensor is due
        (plain, f(V, 3, H, W), None, one),                                                       # [V,3,H,W] from the view callable
        (full, f(V, 3, H, W), tup, tup),                                                         # a bare tensor where a tuple is due
        (full, (f(3, H, W), None, None), tup, tup),                                              # wrong arity
        (full, (f(3, H, W, dt=torch.float64), None, None, None), bare, bare),
        (full, (f(3, H, W), None, f(1, H, W, dt=torch.float64), None),
         f"upstream: dL_ddepth must be None or a float32 GPU tensor {[V, 1, H, W]} or {[1, H, W]}", f"upstream: dL_ddepth must be None or a float32 GPU tensor {[1, H, W]}"),
        (full, (f(3, H, W), None, None, f(1, H, W)),
         f"upstream: dL_dfeatures must be None or a float32 GPU tensor {[V, C, H, W]} or {[C, H, W]}", f"upstream: dL_dfeatures must be None or a float32 GPU tensor {[C, H, W]}"),
        (full, (f(V, 3, H, W), None, None, None), None, one),                                    # [V,3,H,W] from the view callable
    ]
    for c, ret, batch_message, view_message in bad:
        b, w = caller(c, ret)
        m = maps3 if c.names else []
        for ask, message in ((lambda: b.batch(images, m), batch_message), (lambda: b.views(images, m), batch_message),
                             (lambda: w.view(0, images, m), view_message), (lambda: w.views(images, m)(0), view_message)):
            if message is None:
                ask()
            else:
                with pytest.raises(RuntimeError) as e:
                    ask()
                assert str(e.value) == message
    with pytest.raises(RuntimeError, match="GPU"):                                               # the default: a device is required
        _Upstream(plain, lambda images: f(V, 3, H, W), None).batch(images, [])
