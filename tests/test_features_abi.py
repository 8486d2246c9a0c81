"""CPU: the feature-channel extension at the C ABI and the public API (no device needed), and the yardstick the GPU tests of
tests/test_gpu_features.py measure against.

The yardstick: the reference's rasterizer has no feature output, but compositing is linear in colour and it does not clamp precomputed
colours.  For features F[P,C] and each triple of channels (the last one zero-padded), a frame of the SAME geometry with
colors_precomp = F[:, triple], no SH and background 0 IS the feature map's triple.  Under the upstream g[triple] its dL_dcolors is
dL_dfeatures[:, triple], and its dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcov3D, dL_dscales, dL_drotations and dL_dmeans3D -- summed over
the triples, the share being linear in the channels -- are the through-alpha gradients of the feature map."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

from tests import util
from tests.test_depth_abi import _numpy_depth, lib_path
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_features", "tgs_backward_features_opt")
SUMMED = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


def _lib():
    lib = ctypes.CDLL(lib_path())
    vp, it, i64, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    lib.tgs_last_error.restype = ctypes.c_char_p
    lib.tgs_features.restype = it
    lib.tgs_features.argtypes = [vp, it, it, it, it, i64, vp, vp, vp, vp, vp]
    lib.tgs_backward_features_opt.restype = it
    lib.tgs_backward_features_opt.argtypes = [vp, it, vp, it, it, it, i64, vp, it, it, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, fl, fl, vp,
                                              vp, vp, vp, vp, vp, vp, vp, it, vp, vp, vp, vp] + [vp] * 9 + [it]
    return lib


def make_features(P: int, C: int, seed: int = 515) -> np.ndarray:
    """signed standard-normal features: half of the values are negative, as normals are"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((P, C)).astype(np.float32)


def triples(C: int):
    """the channel triples of C channels: [0, 1, 2], [3, 4, 5], ... (the last one may be shorter)"""
    return [list(range(c, min(c + 3, C))) for c in range(0, C, 3)]


def feature_colour_input(inp: dict, F: np.ndarray, cols) -> dict:
    """the same geometry with colours F[:, cols] (zero-padded to three), no SH, over the background 0: its frame is the feature map's triple"""
    d = {k: v for k, v in inp.items() if k != "shs"}
    col = np.zeros((F.shape[0], 3), np.float32)
    col[:, :len(cols)] = np.asarray(F, np.float32)[:, cols]
    d["colors_precomp"] = col
    d["bg"] = np.zeros(3, np.float32)
    return d


def feature_upstream(g: np.ndarray, cols) -> np.ndarray:
    """upstream gradient of that frame which stands for the upstream g[C,H,W] of the feature map: g[cols], zero-padded to three channels"""
    d = np.zeros((3,) + g.shape[1:], np.float32)
    d[:len(cols)] = g[cols]
    return d


def oracle_features(inp: dict, F: np.ndarray, g, variant: str, n_contrib=None):
    """-> feature map [C,H,W], and with an upstream g[C,H,W] dL_dfeatures [P,C] and the through-alpha gradients summed over the triples (float64)"""
    P, C = F.shape
    fmap, dF, summed = [], np.zeros((P, C), np.float64), None
    for cols in triples(C):
        d = util.oracle_run(feature_colour_input(inp, F, cols), None if g is None else feature_upstream(g, cols), variant=variant)
        if n_contrib is not None:
            assert np.array_equal(np.asarray(d["n_contrib"]), n_contrib), "a feature-colour frame blends other pairs than the colour frame"
        fmap.append(np.asarray(d["color"])[:len(cols)])
        if g is not None:
            dF[:, cols] = np.asarray(d["dL_dcolors"], np.float64).reshape(P, 3)[:, :len(cols)]
            t = {k: np.asarray(d[k], np.float64) for k in SUMMED}
            summed = t if summed is None else {k: summed[k] + t[k] for k in SUMMED}
    return np.concatenate(fmap, 0), dF, summed


def test_header_declares_and_library_exports_the_feature_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    assert int(re.search(r"#define TGS_FEATURE_MAX_CHANNELS (\d+)", src).group(1)) == 16
    assert "sum_i T_i(p) * alpha_i(p) * features[i*C + c]" in text and "sum_c g_c * (f_ic - accum_rec_ic)" in text     # the definition and the alpha path
    assert "feature channels are tgs_features below" in text                                                         # the depth comment points here
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

    def fwd(P=10, C=5, W=64, H=64, R=5, geom=some, binning=some, img=some, feat=some, out=some):
        return lib.tgs_features(None, P, C, W, H, R, geom, binning, img, feat, out)
    for kw in (dict(C=0), dict(C=17), dict(C=-2), dict(P=-1), dict(W=0), dict(H=-3), dict(R=-1), dict(geom=None), dict(binning=None), dict(img=None),
               dict(feat=None), dict(out=None)):
        assert fwd(**kw) == INVALID and "tgs_features" in msg(), (kw, msg())

    def bwd(P=10, R=5, W=64, H=64, C=5, geom=some, binning=some, img=some, radii=some, dpix=some, dA=None, dD=None, dz=None, feat=some, dF=some, scratch=some,
            dfeat=some, out=some):
        return lib.tgs_backward_features_opt(None, 0, None, P, 0, 0, R, some, W, H, some, None, some, some, 1.0, some, None, some, some, some, 1.0, 1.0, radii,
                                             geom, binning, img, dpix, dA, dD, dz, C, feat, dF, scratch, dfeat, out, None, out, out, out, None, None, out, out, 0)
    for kw in (dict(C=0), dict(C=17), dict(feat=None), dict(scratch=None), dict(dfeat=None), dict(W=0), dict(R=-1), dict(img=None), dict(dpix=None), dict(radii=None),
               dict(out=None), dict(dD=some, dz=None)):
        assert bwd(**kw) == INVALID and "tgs_backward_features_opt" in msg(), (kw, msg())
    assert bwd(C=17) == INVALID and "17" in msg()
    # without an upstream on the map it is the depth call: the other four arguments are not looked at, and its errors carry its name
    assert bwd(dF=None, C=0, feat=None, scratch=None, dfeat=None, dD=some, dz=None) == INVALID and "tgs_backward_depth_opt" in msg()


def test_empty_model_and_empty_frame_are_no_ops():
    lib = _lib()
    some = ctypes.c_void_p(4096)
    assert lib.tgs_features(None, 0, 5, 64, 64, 0, None, None, None, None, None) == 0
    assert lib.tgs_features(None, 10, 5, 64, 64, 0, some, some, some, some, some) == 0      # a frame without instances: nothing launched, nothing written
    assert lib.tgs_features(None, 10, 16, 64, 64, 0, None, None, None, None, None) == 0
    assert lib.tgs_backward_features_opt(None, 0, None, 0, 0, 0, 0, None, 64, 64, None, None, None, None, 1.0, None, None, None, None, None, 1.0, 1.0, None,
                                         None, None, None, None, None, None, None, 5, None, some, None, None,
                                         None, None, None, None, None, None, None, None, None, 0) == 0


def test_public_api_has_features_defaulting_to_none():
    import diff_gaussian_rasterization as dgr
    for fn in (dgr.GaussianRasterizer.forward, dgr.rasterize_gaussians):
        p = inspect.signature(fn).parameters
        assert "features" in p and p["features"].default is None
        assert p["return_alpha"].default is False and p["return_depth"].default is False
        names = list(p)
        assert names.index("return_alpha") < names.index("return_depth") < names.index("features")
    from diff_gaussian_rasterization import _C
    assert callable(_C.features_from_state)
    doc = _C.rasterize_gaussians_backward.__doc__
    assert "grad_out_features" in doc and "features" in doc and "grad_out_depth" in doc and "grad_out_alpha" in doc
    doc = dgr.rasterize_gaussians.__doc__
    assert doc.index("alpha[1,H,W]") < doc.index("depth[1,H,W]") < doc.index("feature_map[C,H,W]")
    import youreditableavatar_amd.diff_gaussian_rasterization as impl
    assert impl._RasterizeGaussiansAlpha is impl._RasterizeGaussiansExt and impl._RasterizeGaussians is not impl._RasterizeGaussiansExt
    assert "features" in inspect.signature(impl._RasterizeGaussiansExt.forward).parameters


def test_public_api_refuses_bad_features_before_any_device_call():
    import pytest
    import torch
    import diff_gaussian_rasterization as dgr
    means = torch.zeros(7, 3)
    for bad, what in ((torch.zeros(7, 0), "channels"), (torch.zeros(7, 17), "channels"), (torch.zeros(6, 4), "shape"), (torch.zeros(7), "shape"),
                      (torch.zeros(7, 4, dtype=torch.float64), "float32")):
        with pytest.raises(ValueError, match=what):
            dgr.rasterize_gaussians(means, None, None, None, None, None, None, None, None, features=bad)


def test_the_yardstick_itself():
    """On make_cloud(600, 1, 1) at 72x40 with C = 5 signed features: every triple frame blends the colour frame's pairs (same n_contrib and
    final_T); channel 0 IS sum T alpha f over those pairs, recomputed in numpy from the oracle's lists (so the oracle does not clamp
    precomputed colours); and the map, dL_dfeatures and the through-alpha gradients agree with an independent fp64 autograd splat that has
    the features as colors_precomp leaves.  Bounds: 1e-6 for the numpy sum against the fp64 oracle (both double: only the summation order
    differs), 1e-5 for the autograd splat -- the bounds tests/test_depth_abi.py holds the same pair of programs to.  A guard on the
    reference, not on the code under test."""
    import torch
    from oracle import torch_splat
    from youreditableavatar_amd import scenes
    W, H, P, C = 72, 40, 600, 5
    cloud = scenes.make_cloud(P, 1, 1)
    cam = scenes.orbit_camera(W, H, azimuth_deg=30)
    inp = util.scene_input(cloud, cam)
    F = make_features(P, C)
    g = (np.random.Generator(np.random.PCG64(9)).standard_normal((C, H, W)) / (H * W)).astype(np.float32)
    runs = {}
    for variant in ("f32", "f64"):
        col = util.oracle_run(inp, None, variant=variant)
        fmap, dF, summed = oracle_features(inp, F, g, variant, n_contrib=np.asarray(col["n_contrib"]))
        for cols in triples(C):
            d = util.oracle_run(feature_colour_input(inp, F, cols), None, variant=variant)
            assert np.array_equal(np.asarray(d["final_T"]), np.asarray(col["final_T"])), variant
        runs[variant] = (col, fmap, dF, summed)
    col, fmap, dF, summed = runs["f64"]
    assert fmap.shape == (C, H, W) and fmap.min() < 0 < fmap.max(), "signed features give a signed map: nothing is clamped"
    ref = _numpy_depth(col, np.asarray(F[:, 0], np.float64), H, W)
    e = util.rel_l2(fmap[0], ref)
    print(f"channel 0 of the feature-colour frame against sum T alpha f from the oracle's lists: {e:.3e}")
    assert np.abs(ref).max() > 0 and e <= 1e-6
    e = util.rel_l2(runs["f32"][1][0], ref)
    print(f"the fp32 oracle's channel 0 against the same: {e:.3e}")
    assert e <= util.REL_TOL
    for k in SUMMED:
        print(f"{k}: fp32 vs fp64 expectation {util.rel_l2(runs['f32'][3][k], summed[k]):.3e}")
    print(f"dL_dfeatures: fp32 vs fp64 expectation {util.rel_l2(runs['f32'][2], dF):.3e}")
    # the independent fp64 autograd splat: the features are leaves, one splat per triple, one loss
    t = lambda a, rg=False: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=rg)
    leaves = {"means3D": t(cloud["means3D"], True), "means2D": torch.zeros(P, 3, dtype=torch.float64, requires_grad=True), "opacities": t(cloud["opacities"], True),
              "scales": t(cloud["scales"], True), "rotations": t(cloud["rotations"], True)}
    Ft = t(F, True)
    loss, maps = 0.0, []
    for cols in triples(C):
        cp = torch.cat([Ft[:, cols], torch.zeros(P, 3 - len(cols), dtype=torch.float64)], 1)
        color, radii = torch_splat.splat(viewmatrix=t(cam.viewmatrix), projmatrix=t(cam.projmatrix), campos=t(cam.campos), bg=torch.zeros(3, dtype=torch.float64),
                                         tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, image_height=H, image_width=W, sh_degree=0,
                                         scale_modifier=cam.scale_modifier, colors_precomp=cp, **leaves)
        maps.append(color[:len(cols)])
        loss = loss + (color * torch.tensor(feature_upstream(g, cols), dtype=torch.float64)).sum()
    e = util.rel_l2(torch.cat(maps, 0).detach().numpy(), fmap)
    print(f"feature map: fp64 autograd splat vs fp64 oracle {e:.3e}")
    assert e <= 1e-5
    loss.backward()
    e = util.rel_l2(dF, Ft.grad.numpy())
    print(f"dL_dfeatures: expectation from the fp64 oracle vs fp64 autograd splat {e:.3e}")
    assert np.linalg.norm(Ft.grad.numpy()) > 0 and e <= 1e-5
    vis = np.asarray(col["radii"]) > 0
    assert np.all(dF[~vis] == 0), "culled Gaussians have zero feature rows in the expectation"
    expect = {"means3D": summed["dL_dmeans3D"].reshape(P, 3), "means2D": summed["dL_dmeans2D"].reshape(P, 3), "opacities": summed["dL_dopacity"].reshape(P, 1),
              "scales": summed["dL_dscales"].reshape(P, 3), "rotations": summed["dL_drotations"].reshape(P, 4)}
    for k, ex in expect.items():
        got = leaves[k].grad.numpy().reshape(ex.shape)
        if k == "means2D":
            got, ex = got[:, :2], ex[:, :2]
        e = util.rel_l2(ex, got)
        print(f"{k}: through-alpha expectation from the fp64 oracle vs fp64 autograd splat {e:.3e}")
        assert np.linalg.norm(got) > 0 and e <= 1e-5, (k, e)
