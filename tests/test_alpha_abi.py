"""CPU: the accumulated-alpha extension at the C ABI and the public API (no device needed), and the yardstick the GPU tests of
tests/test_gpu_alpha.py measure against.

The yardstick: the reference's rasterizer has no alpha output, but a frame of the SAME geometry with colours 0, background (1, 0, 0) and
upstream gradient (-g_A, 0, 0) has channel 0 == final_T, so its gradients are exactly the gradients of alpha = 1 - final_T under the
upstream g_A.  By linearity a frame with upstream (dL_dpix, g_A) has the gradients
    oracle(inp, dL_dpix) + oracle(zero-colour inp, (-g_A, 0, 0))
for everything but the colour inputs, which alpha does not depend on."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

from tests import util
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_alpha", "tgs_backward_alpha_opt", "tgs_backward_render_alpha_opt")


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it, i64, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_alpha.restype = it
    lib.tgs_alpha.argtypes = [vp, it, it, vp, vp]
    lib.tgs_backward_alpha_opt.restype = it
    lib.tgs_backward_alpha_opt.argtypes = [vp, it, vp, it, it, it, i64, vp, it, it, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, fl, fl, vp,
                                           vp, vp, vp, vp, vp] + [vp] * 9 + [it]
    lib.tgs_backward_render_alpha_opt.restype = it
    lib.tgs_backward_render_alpha_opt.argtypes = [vp, vp, it, i64, vp, it, it, vp, vp, vp, vp]
    return lib


def zero_colour_input(inp: dict) -> dict:
    """the same geometry with colours 0 over the background (1, 0, 0): channel 0 of its frame is final_T"""
    z = {k: v for k, v in inp.items() if k != "shs"}
    z["colors_precomp"] = np.zeros((inp["means3D"].shape[0], 3), np.float32)
    z["bg"] = np.array([1.0, 0.0, 0.0], np.float32)
    return z


def alpha_upstream(g_A: np.ndarray) -> np.ndarray:
    """upstream gradient of the zero-colour frame that stands for the upstream g_A[H,W] of alpha = 1 - channel 0"""
    d = np.zeros((3,) + g_A.shape, np.float32)
    d[0] = -g_A
    return d


def test_header_declares_and_library_exports_the_alpha_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert int(re.search(r"#define TGS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 3
    text = open(HEADER).read()
    assert "1 - final_T" in text and "straight-through" in text          # the definition and the gradient convention are written down
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
    for args in ((None, 64, 64, None, some), (None, 64, 64, some, None), (None, 0, 64, some, some), (None, 64, -3, some, some)):
        assert lib.tgs_alpha(*args) == INVALID and "tgs_alpha" in msg(), (args, msg())

    def bwd(P=10, R=5, W=64, H=64, bg=some, geom=some, binning=some, img=some, radii=some, dpix=some, dA=some, out=some):
        return lib.tgs_backward_alpha_opt(None, 0, None, P, 0, 0, R, bg, W, H, some, None, some, some, 1.0, some, None, some, some, some, 1.0, 1.0, radii,
                                          geom, binning, img, dpix, dA, out, None, out, out, out, None, None, out, out, 0)
    for kw in (dict(W=0), dict(H=-1), dict(R=-1), dict(img=None), dict(binning=None), dict(geom=None), dict(dpix=None), dict(radii=None), dict(out=None)):
        assert bwd(**kw) == INVALID and "tgs_backward_alpha_opt" in msg(), (kw, msg())
    assert bwd(dpix=None, dA=some) == INVALID and "NULL" in msg()        # dL_dpix stays required next to dL_dalpha

    def rbwd(P=10, R=5, W=64, H=64, bg=some, binning=some, img=some, dpix=some, dA=some):
        return lib.tgs_backward_render_alpha_opt(None, None, P, R, bg, W, H, binning, img, dpix, dA)
    for kw in (dict(W=0), dict(H=0), dict(R=-2), dict(P=-1), dict(bg=None), dict(binning=None), dict(img=None), dict(dpix=None)):
        assert rbwd(**kw) == INVALID and "tgs_backward_render_alpha_opt" in msg(), (kw, msg())


def test_empty_model_is_a_no_op_for_both_backward_entry_points():
    lib = _lib()
    assert lib.tgs_backward_render_alpha_opt(None, None, 0, 0, None, 64, 64, None, None, None, None) == 0
    assert lib.tgs_backward_alpha_opt(None, 0, None, 0, 0, 0, 0, None, 64, 64, None, None, None, None, 1.0, None, None, None, None, None, 1.0, 1.0, None,
                                      None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0) == 0


def test_public_api_has_return_alpha_defaulting_to_false():
    import diff_gaussian_rasterization as dgr
    for fn in (dgr.GaussianRasterizer.forward, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "return_alpha" in p and p["return_alpha"].default is False
    from diff_gaussian_rasterization import _C
    assert callable(_C.alpha_from_state)
    assert "grad_out_alpha" in _C.rasterize_gaussians_backward.__doc__ and "grad_out_alpha" in inspect.signature(_C.rasterize_gaussians_backward_render).parameters


def test_the_yardstick_itself():
    """On make_cloud(600, 1, 1): channel 0 of the zero-colour frame IS final_T (its own, and the coloured frame's, bit for bit), and the fp64
    oracle's gradients of it agree with an independent fp64 autograd splat to <= 1e-5 (measured while the feature was specified: <= 1.5e-6;
    a guard on the reference, not on the code under test)."""
    from oracle import torch_splat
    from youreditableavatar_amd import scenes
    W, H = 72, 40
    cloud = scenes.make_cloud(600, 1, 1)
    cam = scenes.orbit_camera(W, H, azimuth_deg=30)
    inp = util.scene_input(cloud, cam)
    zinp = zero_colour_input(inp)
    g_A = (np.random.Generator(np.random.PCG64(7)).standard_normal((H, W)) / (H * W)).astype(np.float32)
    dZ = alpha_upstream(g_A)
    for variant in ("f32", "f64", "f32_fma"):
        col = util.oracle_run(inp, None, variant=variant)
        z = util.oracle_run(zinp, dZ, variant=variant)
        assert np.array_equal(np.asarray(z["color"])[0].astype(np.float32), np.asarray(z["final_T"]).astype(np.float32)), variant
        assert np.array_equal(np.asarray(z["final_T"]), np.asarray(col["final_T"])), variant
        assert np.all(np.asarray(z["color"])[1:] == 0), variant
    zcam = scenes.orbit_camera(W, H, azimuth_deg=30, bg=(1.0, 0.0, 0.0))
    zcloud = dict(cloud, colors_precomp=np.zeros((600, 3), np.float32))
    r = torch_splat.run_scene(zcloud, zcam, dZ, mode="precomp")
    assert util.rel_l2(r["final_T"], z["final_T"]) <= 1e-5          # (z: the f32_fma build, the last of the loop)
    z64 = util.oracle_run(zinp, dZ, variant="f64")
    pairs = [("dL_dmeans3D", "grad_means3D"), ("dL_dmeans2D", "grad_means2D"), ("dL_dopacity", "grad_opacities"), ("dL_dscales", "grad_scales"),
             ("dL_drotations", "grad_rotations")]
    for a, b in pairs:
        e = util.rel_l2(np.asarray(z64[a]).reshape(600, -1), np.asarray(r[b]).reshape(600, -1))
        print(f"{a}: fp64 oracle vs fp64 autograd splat {e:.3e}")
        assert np.linalg.norm(r[b]) > 0 and e <= 1e-5, (a, e)
