"""CPU: the expected-depth extension at the C ABI and the public API (no device needed), and the yardstick the GPU tests of
tests/test_gpu_depth.py measure against.

The yardstick: the reference's rasterizer has no depth output, but compositing is linear in colour.  A frame of the SAME geometry with
colors_precomp = (z, z, z) (z = the oracle's own view-space depths of the colour frame), no SH and background 0 has
channel 0 == depth = sum_i T_i alpha_i z_i.  Under the upstream (g_D, 0, 0) its dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcov3D,
dL_dscales, dL_drotations and dL_dmeans3D are the alpha-path gradients of depth and its dL_dcolors[:, 0] is dL_dz, which reaches
dL_dmeans3D through the third row of the view transform: z = m[2] x + m[6] y + m[10] z + m[14].  So a frame with upstream
(dL_dpix, g_D) has the gradients
    oracle(inp, dL_dpix) + oracle(depth-colour inp, (g_D, 0, 0))      for those seven tensors,
    + dL_dz (x) (m[2], m[6], m[10])                                   added to dL_dmeans3D,
    oracle(inp, dL_dpix) alone                                        for dL_dsh / dL_dcolors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

from tests import util
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_depth", "tgs_backward_depth_opt")


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it, i64, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_depth.restype = it
    lib.tgs_depth.argtypes = [vp, it, it, it, i64, vp, vp, vp, vp]
    lib.tgs_backward_depth_opt.restype = it
    lib.tgs_backward_depth_opt.argtypes = [vp, it, vp, it, it, it, i64, vp, it, it, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, fl, fl, vp,
                                           vp, vp, vp, vp, vp, vp, vp] + [vp] * 9 + [it]
    return lib


def depth_colour_input(inp: dict, z: np.ndarray) -> dict:
    """the same geometry with colours (z, z, z), no SH, over the background 0: channel 0 of its frame is the expected depth"""
    d = {k: v for k, v in inp.items() if k != "shs"}
    d["colors_precomp"] = np.repeat(np.asarray(z, np.float32).reshape(-1, 1), 3, axis=1)
    d["bg"] = np.zeros(3, np.float32)
    return d


def depth_upstream(g_D: np.ndarray) -> np.ndarray:
    """upstream gradient of the depth-colour frame that stands for the upstream g_D[H,W] of depth = its channel 0"""
    d = np.zeros((3,) + g_D.shape, np.float32)
    d[0] = g_D
    return d


def z_row(viewmatrix) -> np.ndarray:
    """d z / d mean for the flat view matrix as the API passes it: (m[2], m[6], m[10])"""
    m = np.asarray(viewmatrix, np.float64).reshape(-1)
    return np.array([m[2], m[6], m[10]], np.float64)


def test_header_declares_and_library_exports_the_depth_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    assert "sum_i T_i * alpha_i * z_i" in text and "m[2] x + m[6] y + m[10] z + m[14]" in text      # the definition and the z chain are written down
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    lib = ctypes.CDLL(lib_path())
    lib.tgs_abi_version.restype = ctypes.c_int
    lib.tgs_sizeof_view.restype = lib.tgs_sizeof_options.restype = ctypes.c_size_t
    assert lib.tgs_abi_version() == 3 and lib.tgs_sizeof_options() == 56 and lib.tgs_sizeof_view() == 192


def test_buffer_size_queries_are_unchanged():
    """the depth pass lives in the state a frame already has: its dz scratch is the caller's, not a part of the binning buffer"""
    lib = ctypes.CDLL(lib_path())
    sizes = (ctypes.c_size_t * 3)()
    lib.tgs_state_sizes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    lib.tgs_state_sizes.restype = None
    lib.tgs_state_sizes(1000, 200, 120, 1, 1, 5000, sizes)
    # the binning buffer: keys 8, tile_of 4, recA 16, recB 16, recC 8, slot 4, qmask 8 and three 16-B slab cells per instance, each array
    # starting on a 256-B boundary, 256 B behind the last
    R, end = 5000, 0
    for b in (8, 4, 16, 16, 8, 4, 8, 48):
        end = ((end + 255) & ~255) + R * b
    assert sizes[1] == end + 256


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some = ctypes.c_void_p(4096)            # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    INVALID = -1

    def depth(P=10, W=64, H=64, R=5, geom=some, binning=some, img=some, out=some):
        return lib.tgs_depth(None, P, W, H, R, geom, binning, img, out)
    for kw in (dict(P=-1), dict(W=0), dict(H=-3), dict(R=-1), dict(geom=None), dict(binning=None), dict(img=None), dict(out=None)):
        assert depth(**kw) == INVALID and "tgs_depth" in msg(), (kw, msg())

    def bwd(P=10, R=5, W=64, H=64, bg=some, geom=some, binning=some, img=some, radii=some, dpix=some, dA=some, dD=some, dz=some, out=some, view=some):
        return lib.tgs_backward_depth_opt(None, 0, None, P, 0, 0, R, bg, W, H, some, None, some, some, 1.0, some, None, view, some, some, 1.0, 1.0, radii,
                                          geom, binning, img, dpix, dA, dD, dz, out, None, out, out, out, None, None, out, out, 0)
    for kw in (dict(W=0), dict(H=-1), dict(R=-1), dict(img=None), dict(binning=None), dict(geom=None), dict(dpix=None), dict(radii=None), dict(out=None),
               dict(dz=None), dict(dz=None, dA=None), dict(view=None)):
        assert bwd(**kw) == INVALID and "tgs_backward_depth_opt" in msg(), (kw, msg())
    assert bwd(dpix=None, dD=some) == INVALID and "NULL" in msg()        # dL_dpix stays required next to dL_ddepth


def test_empty_model_and_empty_frame_are_no_ops():
    lib = _lib()
    some = ctypes.c_void_p(4096)
    assert lib.tgs_depth(None, 0, 64, 64, 0, None, None, None, None) == 0
    assert lib.tgs_depth(None, 10, 64, 64, 0, some, some, some, some) == 0          # a frame without instances: nothing launched, nothing written
    assert lib.tgs_backward_depth_opt(None, 0, None, 0, 0, 0, 0, None, 64, 64, None, None, None, None, 1.0, None, None, None, None, None, 1.0, 1.0, None,
                                      None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0) == 0


def test_public_api_has_return_depth_defaulting_to_false():
    import diff_gaussian_rasterization as dgr
    for fn in (dgr.GaussianRasterizer.forward, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "return_depth" in p and p["return_depth"].default is False
        assert p["return_alpha"].default is False
        names = list(p)
        assert names.index("return_alpha") < names.index("return_depth")
    from diff_gaussian_rasterization import _C
    assert callable(_C.depth_from_state)
    assert "grad_out_depth" in _C.rasterize_gaussians_backward.__doc__ and "grad_out_alpha" in _C.rasterize_gaussians_backward.__doc__
    # the order of the outputs with both flags is written where a caller reads it
    doc = dgr.rasterize_gaussians.__doc__
    assert doc.index("alpha[1,H,W]") < doc.index("depth[1,H,W]")
    # one node for the extended outputs, the plain node untouched
    import youreditableavatar_amd.diff_gaussian_rasterization as impl
    assert impl._RasterizeGaussiansAlpha is impl._RasterizeGaussiansExt and impl._RasterizeGaussians is not impl._RasterizeGaussiansExt


def _numpy_depth(o: dict, z: np.ndarray, H: int, W: int) -> np.ndarray:
    """sum_i T_i alpha_i z_i in float64 from the oracle's own lists: positions 1 .. n_contrib of each pixel, the reference's two cut-offs"""
    m2 = np.asarray(o["means2D"], np.float64).reshape(-1, 2)
    co = np.asarray(o["conic_opacity"], np.float64).reshape(-1, 4)
    rg, pl, nc = np.asarray(o["ranges"]).astype(np.int64), np.asarray(o["point_list"]).astype(np.int64), np.asarray(o["n_contrib"]).astype(np.int64)
    gx = (W + 15) // 16
    out = np.zeros((H, W), np.float64)
    for y in range(H):
        for x in range(W):
            t = (y // 16) * gx + x // 16
            ids = pl[rg[t, 0]:rg[t, 0] + nc[y, x]]
            if len(ids) == 0:
                continue
            dx, dy = m2[ids, 0] - x, m2[ids, 1] - y
            power = -0.5 * (co[ids, 0] * dx * dx + co[ids, 2] * dy * dy) - co[ids, 1] * dx * dy
            alpha = np.minimum(0.99, co[ids, 3] * np.exp(np.minimum(power, 0.0)))
            alpha = np.where((power > 0) | (alpha < 1.0 / 255.0), 0.0, alpha)
            T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]])
            out[y, x] = float((T * alpha * z[ids]).sum())
    return out


def test_the_yardstick_itself():
    """On make_cloud(600, 1, 1) with positive upstream weights: channel 0 of the depth-colour frame IS sum T alpha z over the colour frame's
    pairs (same n_contrib on every pixel; recomputed in numpy from the oracle's lists), dL_dz == dL_dcolors[:, 0], and value and gradients
    -- the z -> means3D chain included -- agree with an independent fp64 autograd splat whose colours are computed from the means inside
    the graph.  Bounds: 1e-6 for the numpy sum against the fp64 oracle (both double: only the summation order differs), 1e-5 for the
    autograd splat (the bound tests/test_alpha_abi.py holds the same pair of programs to).  A guard on the reference, not on the code
    under test."""
    import torch
    from oracle import torch_splat
    from youreditableavatar_amd import scenes
    W, H, P = 72, 40, 600
    cloud = scenes.make_cloud(P, 1, 1)
    cam = scenes.orbit_camera(W, H, azimuth_deg=30)
    inp = util.scene_input(cloud, cam)
    g_D = (np.random.Generator(np.random.PCG64(7)).random((H, W)) + 0.5).astype(np.float32) / (H * W)
    dD = depth_upstream(g_D)
    runs = {}
    for variant in ("f32", "f64"):
        col = util.oracle_run(inp, None, variant=variant)
        z = np.asarray(col["depths"])
        d = util.oracle_run(depth_colour_input(inp, z), dD, variant=variant)
        assert np.array_equal(np.asarray(d["n_contrib"]), np.asarray(col["n_contrib"])), variant
        assert np.array_equal(np.asarray(d["final_T"]), np.asarray(col["final_T"])), variant
        assert np.array_equal(np.asarray(d["color"])[0], np.asarray(d["color"])[1]) and np.array_equal(np.asarray(d["color"])[0], np.asarray(d["color"])[2])
        # only channel 0 has an upstream gradient: its colour gradient is dL_dz, the other channels get none
        dcol = np.asarray(d["dL_dcolors"]).reshape(P, 3)
        assert np.all(dcol[:, 1:] == 0) and np.linalg.norm(dcol[:, 0]) > 0
        runs[variant] = (col, d, z)
    col, d, z = runs["f64"]
    vis = np.asarray(col["radii"]) > 0
    ref = _numpy_depth(col, np.asarray(z, np.float64), H, W)
    e = util.rel_l2(np.asarray(d["color"])[0], ref)
    print(f"depth-colour frame against sum T alpha z from the oracle's lists: {e:.3e}")
    assert ref.max() > 0 and e <= 1e-6
    e = util.rel_l2(np.asarray(runs["f32"][1]["color"])[0], ref)
    print(f"the fp32 oracle's depth-colour frame against the same: {e:.3e}")
    assert e <= util.REL_TOL
    # the independent fp64 autograd splat: z is a function of the means inside the graph
    t = lambda a, g=False: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=g)
    leaves = {"means3D": t(cloud["means3D"], True), "means2D": torch.zeros(P, 3, dtype=torch.float64, requires_grad=True), "opacities": t(cloud["opacities"], True),
              "scales": t(cloud["scales"], True), "rotations": t(cloud["rotations"], True)}
    V = t(cam.viewmatrix)
    zt = (torch.cat([leaves["means3D"], torch.ones(P, 1, dtype=torch.float64)], 1) @ V)[:, 2:3]
    assert util.rel_l2(zt.detach().numpy().reshape(-1)[vis], np.asarray(z, np.float64).reshape(-1)[vis]) <= 1e-12
    color, radii = torch_splat.splat(viewmatrix=V, projmatrix=t(cam.projmatrix), campos=t(cam.campos), bg=torch.zeros(3, dtype=torch.float64),
                                     tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, image_height=H, image_width=W, sh_degree=0,
                                     scale_modifier=cam.scale_modifier, colors_precomp=zt.expand(-1, 3), **leaves)
    e = util.rel_l2(color.detach().numpy()[0], np.asarray(d["color"])[0])
    print(f"depth: fp64 autograd splat vs fp64 oracle {e:.3e}")
    assert e <= 1e-5
    color.backward(torch.tensor(dD, dtype=torch.float64))
    dz = np.asarray(d["dL_dcolors"], np.float64).reshape(P, 3)[:, 0]
    expect = {"means3D": np.asarray(d["dL_dmeans3D"], np.float64).reshape(P, 3) + dz[:, None] * z_row(cam.viewmatrix)[None, :],
              "means2D": np.asarray(d["dL_dmeans2D"], np.float64).reshape(P, 3), "opacities": np.asarray(d["dL_dopacity"], np.float64).reshape(P, 1),
              "scales": np.asarray(d["dL_dscales"], np.float64).reshape(P, 3), "rotations": np.asarray(d["dL_drotations"], np.float64).reshape(P, 4)}
    for k, ex in expect.items():
        got = leaves[k].grad.numpy().reshape(ex.shape)
        if k == "means2D":
            got, ex = got[:, :2], ex[:, :2]
        e = util.rel_l2(ex, got)
        print(f"{k}: expectation from the fp64 oracle vs fp64 autograd splat {e:.3e}")
        assert np.linalg.norm(got) > 0 and e <= 1e-5, (k, e)
    # the z chain is not a rounding-size part of the means' gradient: without it the two would not agree
    without = util.rel_l2(np.asarray(d["dL_dmeans3D"], np.float64).reshape(P, 3), leaves["means3D"].grad.numpy())
    print(f"means3D without the z chain: {without:.3e}")
    assert without > 1e-3
