"""GPU: youreditableavatar_amd.mesh_raster (csrc/tgs_mesh.hip) against the rule as tests/mesh_ref.py restates it.

Bars (all from the reference alone):
  * coverage and ID are compared exactly on every pixel that is not depth-ambiguous (best and second-best fp64 depth within 4 eta_z; at most
    1 % of a scene's covered pixels, asserted on the CPU in tests/test_mesh_ref.py); on an ambiguous pixel the ID is one of the two candidates;
  * u, v and z/w on agreeing pixels are within 4 eta_uv / 4 eta_z of the fp64 values, eta being the helper's own |fp32 - fp64|;
  * interpolate is within 8 * 2^-24 * (|u a0| + |v a1| + |(1 - u - v) a2|) per element of an fp64 evaluation from the device's own rast, and
    exactly 0 on empty pixels;
  * two runs give the same bits; a permutation of the faces gives the same image; a duplicated face gives the lower index.
The GPU tests pass valid indices only (the refusal of bad ones is tests/test_mesh_raster_abi.py's, before any launch)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mesh_ref as M
from tests.util import ROOT

pytestmark = pytest.mark.gpu


def _dr():
    import youreditableavatar_amd.mesh_raster as dr
    return dr


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # (a copy: the cached arrays are read-only)


def _rasterize(pos, tri, W, H):
    dr = _dr()
    rast, none = dr.rasterize(dr.RasterizeCudaContext(), _dev(pos), _dev(tri), (H, W))
    assert none is None and rast.shape == (1, H, W, 4) and rast.dtype == torch.float32 and rast.grad_fn is None
    return rast


@functools.lru_cache(maxsize=None)
def device_rast(name):
    """the device's image of scene ``name`` (rasterized once), read-only numpy [H,W,4]"""
    s = M.scene(name)
    a = _rasterize(s["pos"], s["tri"], s["W"], s["H"])[0].cpu().numpy()
    a.setflags(write=False)
    return a


def _crop(a, window):
    if window is None:
        return a
    x0, y0, x1, y1 = window
    return a[y0:y1, x0:x1]


def _compare(name, got, ref, tri):
    """the bars of the module docstring on one image (already cropped to the reference's window); -> the non-ambiguous mask"""
    ids = got[..., 3].astype(np.int64) - 1
    assert np.array_equal(got[..., 3], np.round(got[..., 3])) and ids.min() >= -1 and ids.max() < len(tri)
    amb = M.ambiguous(ref, tri)
    ok = ~amb
    assert np.array_equal(ids[ok], ref["winner"][ok]), f"{name}: {int((ids[ok] != ref['winner'][ok]).sum())} pixels with another ID"
    assert np.all((ids[amb] == ref["winner"][amb]) | (ids[amb] == ref["second"][amb]))
    empty = ids < 0
    assert np.all(got[empty] == 0)                                             # exactly (0, 0, 0, 0)
    agree = (ids == ref["winner"]) & ~empty
    err_u = np.abs(got[..., 0].astype(np.float64) - ref["u"])[agree]
    err_v = np.abs(got[..., 1].astype(np.float64) - ref["v"])[agree]
    err_z = np.abs(got[..., 2].astype(np.float64) - ref["z"])[agree]
    e_uv, e_z = (float(max(err_u.max(), err_v.max())), float(err_z.max())) if agree.any() else (0.0, 0.0)
    print(f"{name}: {int(agree.sum())} pixels compared, {int(amb.sum())} ambiguous; eta_uv = {ref['eta_uv']:.3e}, kernel's largest u/v error {e_uv:.3e}; "
          f"eta_z = {ref['eta_z']:.3e}, kernel's largest z/w error {e_z:.3e}")
    assert e_uv <= 4.0 * ref["eta_uv"] and e_z <= 4.0 * ref["eta_z"]
    return ok


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_scene_against_the_rule(name):
    s, ref = M.scene(name), M.reference(name)
    got = device_rast(name)
    assert got.shape == (s["H"], s["W"], 4)
    _compare(name, _crop(got, s["window"]), ref, s["tri"])
    if name.startswith("hand_"):                                               # the duplicated faces 9, 10 never win, the dropped ones never appear
        assert set(np.unique(got[..., 3]).tolist()) <= {1.0, 2.0, 9.0}
    if name == "quad_2048":                                                    # beside the crop: the quad covers what its box says and nothing else
        ids = got[..., 3]
        assert np.all(ids[0:2] == 0) and np.all(ids[:, 0:1] == 0) and np.all(ids[2046:] == 0) and ids[1024, 1024] in (1.0, 2.0)
        assert 2038 * 2035 < int((ids > 0).sum()) < 2044 * 2044
    if name == "fullscreen_512":
        assert np.all(got[..., 3] > 0)


def test_no_faces_and_no_vertices_give_zeros():
    dr = _dr()
    pos = _dev(M.scene("hand_7x5")["pos"])
    rast, _ = dr.rasterize(None, pos, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), (5, 7))
    assert rast.shape == (1, 5, 7, 4) and bool((rast == 0).all())
    rast, _ = dr.rasterize(None, torch.zeros((2, 0, 4), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), (5, 7))
    assert rast.shape == (2, 5, 7, 4) and bool((rast == 0).all())
    out, _ = dr.interpolate(torch.ones((pos.shape[0], 2), device="cuda"), rast, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert out.shape == (2, 5, 7, 2) and bool((out == 0).all())
    assert bool((dr.face_ids(rast) == -1).all())


def test_c_abi_with_no_faces_or_no_vertices_writes_zeros():
    """the wrapper answers F = 0 / V = 0 itself; at the C ABI the call clears and resolves: rast is written, all zero"""
    lib = _dr()._lib
    W, H = 33, 17
    pos = _dev(M.scene("hand_33x17")["pos"])
    tri = _dev(M.scene("hand_33x17")["tri"])
    st = torch.cuda.current_stream().cuda_stream
    for V, F, p, t in ((0, 0, None, None), (len(pos), 0, pos.data_ptr(), None), (0, len(tri), None, tri.data_ptr())):
        n = int(lib.tgs_mesh_workspace_bytes(F, W, H))
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        rast = torch.full((H, W, 4), 7.0, device="cuda")
        assert lib.tgs_mesh_rasterize(st, V, F, p, t, W, H, rast.data_ptr(), ws.data_ptr(), n) == 0
        assert bool((rast == 0).all()), (V, F)


def test_row_zero_is_clip_y_minus_one_and_empty_pixels_are_zero():
    pos = np.array([[-1, -1, 0, 1], [1, -1, 0, 1], [0, -0.5, 0, 1]], np.float32)
    pos = M.unambiguous(pos, 8, 8)
    tri = np.array([[0, 1, 2]], np.int32)
    got = _rasterize(pos, tri, 8, 8)[0].cpu().numpy()
    ref = M.rasterize(pos, tri, 8, 8)
    assert np.array_equal(got[..., 3] > 0, ref["winner"] >= 0)
    assert np.nonzero((got[..., 3] > 0).any(axis=1))[0].tolist() == [0, 1]
    assert np.all(got[2:] == 0) and got[2:].tobytes() == bytes(got[2:].nbytes)         # +0.0 in every channel


@pytest.mark.parametrize("name", ["sheets_64x48", "coarse_200x150", "sphere_256", "tiny_256", "fullscreen_512"])
def test_two_runs_give_the_same_bits(name):
    s = M.scene(name)
    again = _rasterize(s["pos"], s["tri"], s["W"], s["H"])[0].cpu().numpy()
    assert again.tobytes() == device_rast(name).tobytes()


@pytest.mark.parametrize("name", ["hand_16x16", "sheets_64x48", "coarse_200x150", "sphere_256", "tiny_256"])
def test_face_order_does_not_matter(name):
    """the rows of tri permuted, the IDs mapped back: the same rast on every non-ambiguous pixel (u, v and z/w bit for bit)"""
    s, ref = M.scene(name), M.reference(name)
    tri = s["tri"]
    perm = np.random.default_rng(3).permutation(len(tri))
    got = _rasterize(s["pos"], tri[perm], s["W"], s["H"])[0].cpu().numpy().copy()
    hit = got[..., 3] > 0
    got[..., 3][hit] = perm[got[..., 3][hit].astype(np.int64) - 1] + 1
    base = device_rast(name)
    ok = ~M.ambiguous(ref, tri)
    dup = (ref["second"] >= 0) & (ref["z_second"] == ref["z"])               # the winner once more under another index: which copy wins follows the order
    same = ok & ~dup
    assert same.sum() >= 0.5 * ok.sum()
    assert got[same].tobytes() == base[same].tobytes()
    assert np.array_equal(got[..., :3][ok], base[..., :3][ok])               # the values of a duplicate are the winner's own
    if dup.any():
        assert np.all(tri[got[..., 3][dup].astype(np.int64) - 1] == tri[base[..., 3][dup].astype(np.int64) - 1])


def test_a_duplicated_face_gives_the_lower_index():
    s = M.scene("grid_97x61")
    tri = np.concatenate([s["tri"], s["tri"][::-1]])                         # every face twice; the copy of face k is face 2F - 1 - k
    got = _rasterize(s["pos"], tri, 97, 61)[0].cpu().numpy()
    assert got.tobytes() == device_rast("grid_97x61").tobytes() and got[..., 3].max() <= len(s["tri"])


def test_a_batch_is_its_images_one_by_one():
    dr = _dr()
    s = M.scene("sheets_64x48")
    other = s["pos"].copy()
    other[:, 0] = -other[:, 0]
    other = M.unambiguous(other, 64, 48)
    rast, _ = dr.rasterize(None, _dev(np.stack([s["pos"], other])), _dev(s["tri"]), (48, 64))
    assert rast.shape == (2, 48, 64, 4)
    assert rast[0].cpu().numpy().tobytes() == device_rast("sheets_64x48").tobytes()
    assert rast[1].cpu().numpy().tobytes() == _rasterize(other, s["tri"], 64, 48)[0].cpu().numpy().tobytes()
    _compare("sheets mirrored", rast[1].cpu().numpy(), M.rasterize(other, s["tri"], 64, 48), s["tri"])
    # per-image attributes [N,V,C], shared ones [1,V,C] and [V,C]
    rng = np.random.default_rng(9)
    a = rng.normal(0, 1, (2, len(other), 3)).astype(np.float32)
    both, _ = dr.interpolate(_dev(a), rast, _dev(s["tri"]))
    for n in range(2):
        one, _ = dr.interpolate(_dev(a[n]), rast[n:n + 1], _dev(s["tri"]))
        assert torch.equal(both[n], one[0])
    shared, _ = dr.interpolate(_dev(a[:1]), rast, _dev(s["tri"]))
    flat, _ = dr.interpolate(_dev(a[0]), rast, _dev(s["tri"]))
    assert torch.equal(shared, flat) and torch.equal(shared[0], both[0]) and shared.shape == (2, 48, 64, 3)


@pytest.mark.parametrize("name,C", [("sphere_256", 1), ("sphere_256", 3), ("sphere_256", 5), ("hand_33x17", 3), ("offscreen_40x24", 5)])
def test_interpolate(name, C):
    dr = _dr()
    s = M.scene(name)
    rast_np = device_rast(name)
    rast = _dev(rast_np)[None]
    V = len(s["pos"])
    attr = (np.random.default_rng(C).normal(0, 3, (V, C)) + 5.0).astype(np.float32)
    want, bound = M.interpolate(attr, rast_np, s["tri"])
    empty = rast_np[..., 3] == 0
    for shape in ((1, V, C), (V, C)):                                         # [N,V,C] and the broadcast [V,C]
        out, none = dr.interpolate(_dev(attr.reshape(shape)), rast, _dev(s["tri"]))
        assert none is None and out.shape == (1, s["H"], s["W"], C) and out.grad_fn is None
        got = out[0].cpu().numpy()
        excess = np.abs(got.astype(np.float64) - want) - bound
        print(f"{name} C={C} {shape}: largest error {np.abs(got - want).max():.3e}, largest error - bound {excess.max():.3e}")
        assert np.all(excess <= 0)
        assert np.all(got[empty] == 0)
    if name == "sphere_256":
        assert empty.any() and not empty.all()


def test_face_ids_and_hit_faces():
    dr = _dr()
    s, ref = M.scene("sphere_256"), M.reference("sphere_256")
    rast = _dev(device_rast("sphere_256"))[None]
    ids = dr.face_ids(rast)
    assert ids.dtype == torch.int32 and ids.shape == (1, 256, 256) and np.array_equal(ids[0].cpu().numpy(), ref["winner"])
    mask = torch.zeros((256, 256), dtype=torch.bool, device="cuda")
    mask[100:140, 90:170] = True
    hit = dr.hit_faces(rast, mask, num_faces=len(s["tri"]))
    want = np.zeros(len(s["tri"]), bool)
    w = ref["winner"][100:140, 90:170]
    want[w[w >= 0]] = True
    assert hit.dtype == torch.bool and np.array_equal(hit.cpu().numpy(), want) and want.any()
    assert not bool(dr.hit_faces(rast, torch.zeros_like(mask), num_faces=len(s["tri"])).any())


def test_example_runs_and_its_hit_faces_are_the_references():
    spec = importlib.util.spec_from_file_location("mesh_masks_example", os.path.join(ROOT, "examples", "mesh_masks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    r = mod.run(log=lines.append)
    assert lines and "faces hit" in lines[0]
    H, W = r["rect"].shape
    ref = M.rasterize(r["pos"], r["tri"], W, H)
    assert not M.ambiguous(ref, r["tri"]).any()
    w = ref["winner"][r["rect"]]
    want = np.zeros(len(r["tri"]), bool)
    want[w[w >= 0]] = True
    assert np.array_equal(r["hit"], want)
    assert np.array_equal(r["rast"][..., 3].astype(np.int64) - 1, ref["winner"])
