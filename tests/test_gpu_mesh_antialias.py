"""GPU: youreditableavatar_amd.mesh_raster_aa (csrc/tgs_mesh_aa.hip) against the rule as tests/mesh_aa_ref.py restates it.

Bars (all from the restatement alone):
  * the topology equals the dictionary's entry by entry;
  * with the CPU reference's rast uploaded (depth comparisons see identical bits), the set of pixels that differ from ``color`` equals the set
    of pixels that receive a contribution, untouched pixels are bit-equal to ``color``, touched pixels are within 4 eta_aa of the fp64 result
    (eta_aa: the restatement's own |fp32 - fp64|); where the fp32 restatement is bit-equal to the fp64 one the bar is equality with it;
  * two runs give the same bits; a batch equals its images one by one; a passed topology gives the same bits as None.
eta_aa per scene (C = 3; measured by tests/test_mesh_aa_ref.py, which also shows that the scenes are not vacuous) is in INTEGRATION.md 4k."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mesh_aa_ref as R
from tests import mesh_ref as M
from tests.util import ROOT

pytestmark = pytest.mark.gpu


def _dr():
    import youreditableavatar_amd.mesh_raster_aa as dr
    return dr


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # (a copy: the cached arrays are read-only)


def _antialias(color, rast, pos, tri, **kw):
    """one image [H,W,C] -> numpy [H,W,C]"""
    out = _dr().antialias(_dev(color)[None], _dev(rast)[None], _dev(pos), _dev(tri), **kw)
    assert isinstance(out, torch.Tensor) and out.shape == (1,) + color.shape and out.dtype == torch.float32 and out.grad_fn is None
    return out[0].cpu().numpy()


def _compare(label, got, color, ref, random_colors=True):
    """the bars of the module docstring on one image.  With a random colour per pixel every contribution changes its pixel (asserted on the CPU
    for the scenes' colours), so the pixels that differ from ``color`` are the pixels that receive; with a 0 / 1 mask a contribution between
    two equal colours is zero, and the changed pixels are a subset."""
    changed = (got.view(np.uint32) != color.view(np.uint32)).any(axis=-1)
    t = ref["touched"]
    if random_colors:
        assert np.array_equal(changed, t), f"{label}: {int((changed != t).sum())} pixels in one set only"
    assert not changed[~t].any()                                             # untouched pixels are bit-equal to color
    exact = np.array_equal(ref["out32"].astype(np.float64), ref["out64"])
    err = float(np.abs(got[t].astype(np.float64) - ref["out64"][t]).max()) if t.any() else 0.0
    print(f"{label}: {int(t.sum())} touched pixels, eta_aa = {ref['eta_aa']:.3e}, kernel's largest error {err:.3e}" + (" (fp32 restatement exact: equality asked)" if exact else ""))
    if exact:
        assert np.array_equal(got, ref["out32"])
    else:
        assert err <= 4.0 * ref["eta_aa"]


@functools.lru_cache(maxsize=None)
def device_topology(name):
    s = R.scene(name)
    tri = _dev(s["tri"])
    topo = _dr().antialias_construct_topology_hash(tri, num_vertices=len(s["pos"]))
    assert topo.dtype == torch.int32 and topo.shape == (len(s["tri"]), 3) and topo.device == tri.device
    return topo


EXTRA_TRI = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 7], [5, 6, 7], [0, 0, 1], [0, 1, 9], [2, 1, 8], [-1, 2, 3]], np.int32)     # fan, duplicate, bad rows


@pytest.mark.parametrize("name", ["hand_16x16", "sheets_64x48", "sphere_256", "flaps_64x48", "tinypatch_128"])
def test_topology_against_the_dictionary(name):
    s = R.scene(name)
    dr = _dr()
    want = R.topology(s["tri"], len(s["pos"]))
    tri = _dev(s["tri"])
    got = dr.antialias_construct_topology_hash(tri, num_vertices=len(s["pos"]))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(dr.antialias_construct_topology_hash(tri, num_vertices=len(s["pos"])), got)          # two builds, the same bits
    assert torch.equal(dr.antialias_construct_topology_hash(tri), got)                                       # valid indices: V does not matter
    if name == "sheets_64x48":
        assert (want == -1).any() and (want >= 0).any()                      # open boundaries
    if name == "sphere_256":
        assert (want >= 0).all()                                             # closed


def test_topology_of_a_fan_a_duplicate_and_unusable_rows():
    dr = _dr()
    want = R.topology(EXTRA_TRI, 9)
    assert (want == -2).sum() == 3 and want[3].tolist() == [7, 5, 6]
    got = dr.antialias_construct_topology_hash(_dev(EXTRA_TRI), num_vertices=9)
    assert np.array_equal(got.cpu().numpy(), want)
    # without V the row with index 9 counts as a triangle: the edge 0-1 has one neighbour more (still -2), its own row is no longer -1
    loose = dr.antialias_construct_topology_hash(_dev(EXTRA_TRI)).cpu().numpy()
    assert np.array_equal(loose, R.topology(EXTRA_TRI, 1 << 30))
    empty = dr.antialias_construct_topology_hash(torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert empty.shape == (0, 3) and empty.dtype == torch.int32


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("name", R.GPU_SCENES)
def test_scene_against_the_rule(name, C):
    s, ref = R.scene(name), R.reference(name, C)
    color = R.colors(name, C)
    got = _antialias(color, R.scene_rast(name), s["pos"], s["tri"], topology_hash=device_topology(name))
    _compare(f"{name} C={C}", got, color, ref)


@pytest.mark.parametrize("vertical", [True, False])
def test_the_hand_computed_edges(vertical):
    for x, want_p, want_q in ((3.75, 0.75, 0.0), (4.25, 1.0, 0.25)):
        pos, tri, rast, color = R.edge_case(x, vertical)
        got = _antialias(color, rast, pos, tri)[..., 0]
        o = got if vertical else got.T
        assert np.all(o[:, 3] == want_p) and np.all(o[:, 4] == want_q) and np.all(o[:, :3] == 1) and np.all(o[:, 5:] == 0)


def test_the_hand_computed_quads_and_the_smallest_images():
    color = np.random.default_rng(5).uniform(0, 1, (10, 12, 2)).astype(np.float32)
    for folded in (False, True):
        pos, tri, rast = R.quad_case(folded)
        ref = R.antialias(color, rast, pos, tri)
        got = _antialias(color, rast, pos, tri)
        _compare(f"quad folded={folded}", got, color, ref)
        assert bool(got[5, 6, 0] != color[5, 6, 0]) == folded                # the pixel beyond the shared edge
        assert got[4, 6].tobytes() == color[4, 6].tobytes()
    for W, H in ((1, 1), (2, 1), (1, 2)):
        pos, tri, rast, c = R.edge_case(0.75, vertical=W >= H, W=W, H=H)
        got = _antialias(c, rast, pos, tri)
        assert got.reshape(-1).tolist() == ([1.0] if W * H == 1 else [0.75, 0.0])


def test_rasterize_interpolate_antialias_on_the_sphere():
    """device rasterize -> interpolate (a vertex mask) -> antialias: the thresholded mask grows, by at most one pixel, and equals the rule applied
    to the device's own rast"""
    dr = _dr()
    s = M.scene("sphere_256")
    pos, tri = _dev(s["pos"]), _dev(s["tri"])
    vmask = (s["verts"][:, 0] > 0.1).astype(np.float32)[:, None]             # the vertices of one side: a boundary inside the silhouette as well
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos[None], tri, (256, 256))
    mask, _ = dr.interpolate(_dev(vmask), rast, tri)
    out = dr.antialias(mask, rast, pos[None], tri)
    assert out.shape == (1, 256, 256, 1)
    ref = R.antialias(mask[0].cpu().numpy(), rast[0].cpu().numpy(), s["pos"], s["tri"])
    _compare("sphere end to end", out[0].cpu().numpy(), mask[0].cpu().numpy(), ref, random_colors=False)
    before, after = (mask[0, ..., 0] > 0).cpu().numpy(), (out[0, ..., 0] > 0).cpu().numpy()
    grown = before.copy()
    grown[1:] |= before[:-1]; grown[:-1] |= before[1:]; grown[:, 1:] |= before[:, :-1]; grown[:, :-1] |= before[:, 1:]
    assert np.all(after >= before) and np.all(grown >= after)
    assert np.array_equal(after, ref["out32"][..., 0] > 0)
    print(f"sphere end to end: the blend adds {int(after.sum() - before.sum())} mask pixels to {int(before.sum())}")


@pytest.mark.parametrize("name", ["flaps_64x48", "sphere_256", "tinypatch_128"])
def test_two_runs_give_the_same_bits_and_a_passed_topology_changes_nothing(name):
    s, color = R.scene(name), R.colors(name, 3)
    a = _antialias(color, R.scene_rast(name), s["pos"], s["tri"])
    b = _antialias(color, R.scene_rast(name), s["pos"], s["tri"])
    c = _antialias(color, R.scene_rast(name), s["pos"], s["tri"], topology_hash=device_topology(name), pos_gradient_boost=4.0)
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_a_batch_is_its_images_one_by_one():
    dr = _dr()
    s = R.scene("flaps_64x48")
    other = s["pos"].copy()
    other[:, 0] = -other[:, 0]
    other = M.unambiguous(other, 64, 48)
    tri = _dev(s["tri"])
    rasts = np.stack([R.scene_rast("flaps_64x48"), R.rast_of(M.rasterize(other, s["tri"], 64, 48))])
    colors = np.random.default_rng(7).uniform(0, 1, (2, 48, 64, 3)).astype(np.float32)
    both = dr.antialias(_dev(colors), _dev(rasts), _dev(np.stack([s["pos"], other])), tri)
    assert both.shape == (2, 48, 64, 3)
    for n, p in enumerate((s["pos"], other)):
        one = _antialias(colors[n], rasts[n], p, s["tri"])
        assert both[n].cpu().numpy().tobytes() == one.tobytes()
        _compare(f"batch image {n}", one, colors[n], R.antialias(colors[n], rasts[n], p, s["tri"]))
    # shared positions [1,V,4] and [V,4]
    shared = dr.antialias(_dev(colors), _dev(np.stack([rasts[0], rasts[0]])), _dev(s["pos"])[None], tri)
    flat = dr.antialias(_dev(colors), _dev(np.stack([rasts[0], rasts[0]])), _dev(s["pos"]), tri)
    assert torch.equal(shared, flat) and torch.equal(shared[0], both[0])


def test_no_faces_or_no_vertices_copy_color():
    dr = _dr()
    color = _dev(np.random.default_rng(2).uniform(0, 1, (2, 5, 7, 3)).astype(np.float32))
    rast = torch.zeros((2, 5, 7, 4), device="cuda")
    rast[0, 2, 3, 3] = 1.0
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    out = dr.antialias(color, rast, _dev(M.scene("hand_7x5")["pos"]), none)
    assert out.data_ptr() != color.data_ptr() and torch.equal(out, color)
    out = dr.antialias(color, rast, torch.zeros((0, 4), device="cuda"), torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda"))
    assert torch.equal(out, color)
    wrong = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="topology"):
        dr.antialias(color, rast, _dev(M.scene("hand_7x5")["pos"]), none, topology_hash=wrong)
    with pytest.raises(RuntimeError, match="topology"):                      # the right shape on the wrong device
        dr.antialias(color, rast, _dev(M.scene("hand_7x5")["pos"]), none, topology_hash=torch.zeros((0, 3), dtype=torch.int32))


def test_example_runs_and_its_mask_is_the_rules():
    spec = importlib.util.spec_from_file_location("mesh_masks_antialias_example", os.path.join(ROOT, "examples", "mesh_masks_antialias.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    r = mod.run(log=lines.append)
    assert lines and "mask pixels" in lines[-1]
    ref = R.antialias(r["mask"], r["rast"], r["pos"], r["tri"])
    _compare("example", r["mask_aa"], r["mask"], ref, random_colors=False)
    assert r["added"] == int((ref["out32"][..., 0] > 0).sum() - (r["mask"][..., 0] > 0).sum()) and r["added"] > 0
