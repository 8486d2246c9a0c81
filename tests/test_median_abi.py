"""CPU: the median-depth extension at the C ABI and the public API (no device needed), and the yardstick the GPU tests of
tests/test_gpu_median.py measure against.

Definition: over the (pixel, entry) pairs the colour frame blended, front to back, T starts at 1 and becomes T * (1 - alpha) after each
blended pair; the median entry of a pixel is the FIRST blended pair after which T < 0.5 (strict).  median_depth is the view-space z of
that entry, median_index its Gaussian index; a pixel whose T never falls below 0.5 has 0 and -1.

The yardstick is computed from the reference alone: the oracle's state of the colour frame (point_list, ranges, n_contrib, means2D,
conic_opacity, depths) and a NumPy walk per tile that restates the definition -- forward.cu's power, the two cut-offs (power > 0,
alpha < 1/255), the min(0.99, .) clamp, T <- T (1 - alpha), the first T < 0.5 -- in float32 on the fp32 oracle's state and in float64 on
the fp64 oracle's.  Maps are compared by Gaussian index, never by list position.

A pixel is AMBIGUOUS, and left out of index / depth comparisons, if the two walks disagree on its median index, or if in the fp32 walk
some blended pair leaves |T - 0.5| < 0.5e-4 (a relative 1e-4, the project's REL_TOL): a one-ulp difference in exp may then decide the
pixel the other way.  At most 0.5 % of a scene's pixels may be ambiguous: a condition of the test, asserted here for all ten scenes."""
import ctypes
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_median", "tgs_backward_median")
AMBIGUOUS_BAND = 0.5 * util.REL_TOL      # |T - 0.5| below this after a blended pair: the pixel may go either way
AMBIGUOUS_CAP = 0.005                    # of a scene's pixels


def scenes():
    from tests import test_gpu_alpha as A
    return A.SCENES


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_median.restype = it
    lib.tgs_median.argtypes = [vp, it, it, it, i64, vp, vp, vp, vp, vp, vp]
    lib.tgs_backward_median.restype = it
    lib.tgs_backward_median.argtypes = [vp, it, it, it, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


# ---- the yardstick ----
def median_walk(o: dict, H: int, W: int, dtype) -> dict:
    """The definition, per tile, in ``dtype`` arithmetic on the oracle state ``o``: -> index[H,W] (int64, -1: none), depth[H,W] (dtype),
    final_T[H,W] (T behind the last blended pair), near[H,W] (some blended pair left |T - 0.5| < AMBIGUOUS_BAND) and at_first[H,W] (the
    median entry is the pixel's first blended pair)."""
    f = dtype
    m2 = np.asarray(o["means2D"], f).reshape(-1, 2)
    co = np.asarray(o["conic_opacity"], f).reshape(-1, 4)
    z = np.asarray(o["depths"], f).reshape(-1)
    rg, pl = np.asarray(o["ranges"]).astype(np.int64).reshape(-1, 2), np.asarray(o["point_list"]).astype(np.int64)
    nc = np.asarray(o["n_contrib"]).astype(np.int64).reshape(H, W)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    index = np.full((H, W), -1, np.int64)
    depth, final_T, near, at_first = np.zeros((H, W), f), np.ones((H, W), f), np.zeros((H, W), bool), np.zeros((H, W), bool)
    half, one = f(0.5), f(1.0)
    for t in range(gx * gy):
        ty, tx = divmod(t, gx)
        ys, xs = np.meshgrid(np.arange(16 * ty, min(16 * ty + 16, H)), np.arange(16 * tx, min(16 * tx + 16, W)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        n = int(nc[ys, xs].max())                            # the deepest position any pixel of the tile blended
        if rg[t, 1] == rg[t, 0] or n == 0:
            continue
        ids = pl[rg[t, 0]:rg[t, 0] + n]
        dx = m2[ids, 0][None, :] - xs.astype(f)[:, None]     # forward.cu: d = xy - pixf
        dy = m2[ids, 1][None, :] - ys.astype(f)[:, None]
        cx, cy, cz, op = co[ids, 0][None, :], co[ids, 1][None, :], co[ids, 2][None, :], co[ids, 3][None, :]
        power = f(-0.5) * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
        alpha = np.minimum(f(0.99), op * np.exp(np.minimum(power, f(0.0))))
        blended = (np.arange(n)[None, :] < nc[ys, xs][:, None]) & ~((power > 0) | (alpha < f(1.0 / 255.0)))
        T = np.cumprod(np.where(blended, one - alpha, one).astype(f), axis=1, dtype=f)       # T behind each position, sequential in f
        below = blended & (T < half)
        has = below.any(axis=1)
        first = below.argmax(axis=1)
        index[ys[has], xs[has]] = ids[first[has]]
        depth[ys[has], xs[has]] = z[ids[first[has]]]
        final_T[ys, xs] = T[:, -1]
        near[ys, xs] = (blended & (np.abs(T - half) < f(AMBIGUOUS_BAND))).any(axis=1)
        at_first[ys, xs] = has & (first == blended.argmax(axis=1))
    return dict(index=index, depth=depth, final_T=final_T, near=near, at_first=at_first)


@functools.lru_cache(maxsize=None)
def yardstick(name: str) -> dict:
    """-> per scene (computed once, read-only): the fp32 and the fp64 walk on the two oracle builds' states of the colour frame, the
    ambiguous pixels, and the oracle's own final_T / depths / radii"""
    from tests import test_gpu_alpha as A
    inp = A._input(name)
    H, W = int(inp["image_height"]), int(inp["image_width"])
    out = dict(inp=inp, H=H, W=W)
    for variant, dtype in (("f32", np.float32), ("f64", np.float64)):
        o = util.oracle_run(inp, None, variant=variant)
        out[variant] = median_walk(o, H, W, dtype)
        out["final_T_" + variant] = np.asarray(o["final_T"]).reshape(H, W)
        out["depths_" + variant] = np.asarray(o["depths"]).reshape(-1)
        if variant == "f32":
            out["radii"] = np.asarray(o["radii"])
    out["ambiguous"] = (out["f32"]["index"] != out["f64"]["index"]) | out["f32"]["near"]
    for a in (out["ambiguous"], out["f32"]["index"], out["f32"]["depth"]):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", scenes())
def test_the_yardstick_itself(name):
    """A guard on the reference, not on the code under test: the cap on ambiguous pixels, the agreement of the two walks on the others,
    and that each walk replays the frame (its final T is the oracle's final_T to 2e-7)."""
    y = yardstick(name)
    H, W = y["H"], y["W"]
    amb = y["ambiguous"]
    i32, i64 = y["f32"]["index"], y["f64"]["index"]
    print(f"{name}: {int(amb.sum())} ambiguous pixels of {H * W} ({int((i32 != i64).sum())} by disagreement of the walks), "
          f"{int((i32 >= 0).sum())} pixels with a median entry")
    assert amb.sum() <= AMBIGUOUS_CAP * H * W
    ok = ~amb
    assert np.array_equal(i32[ok], i64[ok])
    assert util.rel_l2(y["f32"]["depth"][ok], y["f64"]["depth"][ok]) <= util.REL_TOL
    for variant in ("f32", "f64"):
        d = float(np.abs(y[variant]["final_T"].astype(np.float64) - y["final_T_" + variant].astype(np.float64)).max())
        print(f"{name}: final T of the {variant} walk against the oracle's final_T: max abs {d:.3e}")
        assert d <= 2e-7
    # what a median entry is: no entry exactly where the frame's final T stays at or above one half (the walk's own T)
    assert np.array_equal(i32 >= 0, y["f32"]["final_T"] < np.float32(0.5))
    vis = y["radii"] > 0
    assert np.all(vis[i32[i32 >= 0]]), "a culled Gaussian cannot be a median entry"
    if name == "g10_all_culled":
        assert not vis.any() and np.all(i32 == -1) and np.all(y["f32"]["depth"] == 0)
    else:
        assert (i32 >= 0).any()
    if name in ("cloud_1500_opaque", "g08_opaque_termination"):
        # opaque splats: on some pixel the FIRST blended entry crosses one half (through the 0.99 clamp: T = 0.01)
        assert y["f32"]["at_first"].any() and y["f64"]["at_first"].any()


# ---- the C ABI ----
def test_header_declares_and_library_exports_the_median_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    assert "FIRST blended pair after which T < 0.5" in text and "(m[2], m[6], m[10])" in text      # the definition and the z chain are written down
    assert "No median / mode depth" not in text                                                    # the old sentence is gone
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    lib = ctypes.CDLL(lib_path())
    lib.tgs_abi_version.restype = ctypes.c_int
    lib.tgs_sizeof_view.restype = lib.tgs_sizeof_options.restype = ctypes.c_size_t
    assert lib.tgs_abi_version() == 3 and lib.tgs_sizeof_options() == 56 and lib.tgs_sizeof_view() == 192


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some = ctypes.c_void_p(4096)            # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    INVALID = -1

    def fwd(P=10, W=64, H=64, R=5, geom=some, binning=some, img=some, depth=some, index=some, pos=some):
        return lib.tgs_median(None, P, W, H, R, geom, binning, img, depth, index, pos)
    for kw in (dict(P=-1), dict(W=0), dict(H=-3), dict(R=-1), dict(geom=None), dict(binning=None), dict(img=None), dict(depth=None), dict(index=None), dict(pos=None)):
        assert fwd(**kw) == INVALID and "tgs_median" in msg(), (kw, msg())

    def bwd(P=10, W=64, H=64, R=5, geom=some, binning=some, img=some, view=some, radii=some, pos=some, g=some, dz=some, out=some):
        return lib.tgs_backward_median(None, P, W, H, R, geom, binning, img, view, radii, pos, g, dz, out)
    for kw in (dict(P=-1), dict(W=0), dict(H=-1), dict(R=-1), dict(geom=None), dict(binning=None), dict(img=None), dict(view=None), dict(radii=None), dict(pos=None),
               dict(g=None), dict(dz=None), dict(out=None)):
        assert bwd(**kw) == INVALID and "tgs_backward_median" in msg(), (kw, msg())


def test_empty_model_and_empty_frame_are_no_ops():
    lib = _lib()
    some = ctypes.c_void_p(4096)
    assert lib.tgs_median(None, 0, 64, 64, 0, None, None, None, None, None, None) == 0
    assert lib.tgs_median(None, 10, 64, 64, 0, some, some, some, some, some, some) == 0          # a frame without instances: nothing launched, nothing written
    assert lib.tgs_backward_median(None, 0, 64, 64, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.tgs_backward_median(None, 10, 64, 64, 0, some, some, some, some, some, some, some, some, some) == 0


# ---- binding and public API ----
def test_binding_and_public_api_have_the_median():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    assert callable(_C.median_from_state)
    doc = _C.rasterize_gaussians_backward.__doc__
    assert "grad_out_median" in doc and "median_pos" in doc and "grad_out_depth" in doc and "grad_out_features" in doc
    p = inspect.signature(_C.rasterize_gaussians_backward_accumulate).parameters
    for k in ("grad_out_median", "median_pos"):
        assert k in p and p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (dgr.GaussianRasterizer.forward, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "return_median" in p and p["return_median"].default is False
        assert p["return_alpha"].default is False and p["return_depth"].default is False and p["features"].default is None
    # the order of the outputs is written where a caller reads it, and so is where the gradient goes
    doc = dgr.rasterize_gaussians.__doc__
    assert doc.index("alpha[1,H,W]") < doc.index("depth[1,H,W]") < doc.index("median_depth[1,H,W]") < doc.index("median_index[1,H,W]") < doc.index("feature_map[C,H,W]")
    assert "positions alone" in doc
    import youreditableavatar_amd.diff_gaussian_rasterization as impl
    assert impl._RasterizeGaussians is not impl._RasterizeGaussiansExt
    assert "want_median" in inspect.signature(impl._RasterizeGaussiansExt.forward).parameters
    assert "want_median" not in inspect.signature(impl._RasterizeGaussians.forward).parameters          # the plain node is untouched


def test_the_docs_say_what_the_median_moves_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4h" in text or "### 4h" in text
    sec = text[text.index("4h"):]
    for what in ("return_median", "median_index", "_face_indices[median_index]", "run_views", "rasterize_accumulate", "mode depth"):
        assert what in sec, what
    assert "Not covered: median depth" not in text
