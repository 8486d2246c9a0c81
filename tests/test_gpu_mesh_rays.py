"""GPU: the mesh ray casting (youreditableavatar_amd.mesh_rays, csrc/tgs_mesh_rays.hip) against the float64 restatement (tests/mesh_rays_ref.py) under
the bars of ``mesh_rays_ref.check_bars``, the tree walk against the walk over every face bit for bit, two runs bit for bit, the launch shapes around a
wave, exact ties and seams, the hit-face array, occlusion, ``from_sdf`` and the module's call shapes.  The body mesh comes from
tests/golden/ref_mesh_sdf_fixture.npz; every scene's rays and reference come from ``mesh_rays_ref.scene``, computed once."""
import numpy as np
import pytest
import torch

from tests import mesh_rays_ref as M
from tests import mesh_sdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("t_hit", "primitive_ids", "geometry_ids", "primitive_uvs", "primitive_normals")
_scenes = {}


def scene(name):
    """-> (vertices, faces, rays, the restatement's outputs, the RaycastingScene on the device)"""
    from youreditableavatar_amd.mesh_rays import RaycastingScene
    if name not in _scenes:
        v, f, rays, ref = M.scene(name)
        _scenes[name] = (v, f, rays, ref, RaycastingScene(to_dev(v), to_dev(f)))
    return _scenes[name]


def to_dev(a):
    """a numpy array (the shared ones are read-only) -> a tensor on the device"""
    return torch.tensor(a, device=DEV)


def run(sc, rays, mode):
    """-> (t_hit, primitive_ids, geometry_ids, uvs, normals) as numpy arrays"""
    out = sc.cast_rays(rays, mode=mode)
    assert tuple(out) == ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals")
    return tuple(out[k].cpu().numpy() for k in KEYS)


def same_bits(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def bars(v, f, rays, ref, out, what):
    t, face, geom, uv, normal = out
    assert np.array_equal(geom.reshape(-1), np.where(face.reshape(-1) >= 0, 0, -1))
    return M.check_bars(v, f, rays, ref, t, face, uv, normal, what=what)


@pytest.mark.parametrize("name", M.scene_names())
def test_scene_against_the_restatement_and_mode_0_against_mode_1(name):
    v, f, rays, ref, sc = scene(name)
    assert sc.device == torch.device(DEV)
    r = to_dev(rays)
    walk, brute = run(sc, r, 0), run(sc, r, 1)
    assert same_bits(walk, brute)                                               # equal bits of every output
    assert same_bits(walk, run(sc, r, 0)) and same_bits(brute, run(sc, r, 1))   # two runs give equal bits
    bars(v, f, rays, ref, walk, name)
    t, face, geom, uv, normal = walk
    assert np.isposinf(t[-3:]).all() and (face[-3:] == -1).all() and (geom[-3:] == -1).all() and not uv[-3:].any() and not normal[-3:].any()      # the invalid rays
    if name == "body":
        assert (face >= 0).sum() >= 40 and (face < 0).sum() >= 40               # both hits and misses occur


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("name", ["body", "cube"])
def test_launch_shapes(name, n):
    v, f, rays, ref, sc = scene(name)
    take = np.arange(n) % len(rays)                                             # 4 097 rays from 386: the scene's rays over and over
    rays, ref = rays[take], {k: a[take] for k, a in ref.items()}
    r = to_dev(rays)
    walk, brute = run(sc, r, 0), run(sc, r, 1)
    assert [a.shape for a in walk] == [(n,), (n,), (n,), (n, 2), (n, 3)] and walk[1].dtype == np.int32 and walk[2].dtype == np.int32
    assert same_bits(walk, brute)
    if n:
        bars(v, f, rays, ref, walk, f"{name} N={n}")
    occ = sc.test_occlusions(r)
    assert occ.shape == (n,) and occ.dtype == torch.bool and torch.equal(occ, sc.test_occlusions(r, mode=1))
    assert sc.hit_faces(r).shape == (len(f),)


@pytest.mark.parametrize("name", ["body", "cube"])
def test_ray_array_shapes(name):
    v, f, rays, ref, sc = scene(name)
    rays, ref = rays[:384], {k: a[:384] for k, a in ref.items()}
    flat = run(sc, to_dev(rays), 0)
    for shape in ((1, 384, 6), (16, 24, 6)):                                    # the reference's [1, M, 6], and an image's [H, W, 6]
        r = to_dev(rays.reshape(shape))
        for mode in (0, 1):
            out = run(sc, r, mode)
            assert [a.shape for a in out] == [shape[:2], shape[:2], shape[:2], shape[:2] + (2,), shape[:2] + (3,)]
            assert same_bits([a.reshape(b.shape) for a, b in zip(out, flat)], flat)
        bars(v, f, rays, ref, out, f"{name} {shape}")
        assert sc.test_occlusions(r).shape == shape[:2]
    wide = to_dev(np.concatenate([rays, rays[::-1]], axis=1))     # a view that is not contiguous: every other block of six
    assert not wide[:, :6].is_contiguous()
    for mode in (0, 1):
        assert same_bits(run(sc, wide[:, :6], mode), flat)
    assert same_bits(run(sc, to_dev(rays)[::3], 0), [np.ascontiguousarray(a[::3]) for a in flat])


def test_tree_shapes():
    for name, nodes in (("triangle", 1), ("one_leaf", 1), ("one_leaf_and_one", 3)):
        sc = scene(name)[4]
        assert int(sc._sdf._tree[:64].view(np.uint32)[2]) == nodes, name


def test_watertight_on_the_device():
    v, f, _, _, sc = scene("cube")
    rays, want_t = M.cube_tie_rays()
    ref = M.cast(v, f, rays)
    for mode in (0, 1):
        t, face, _, _, _ = run(sc, to_dev(rays), mode)
        assert np.array_equal(t, want_t.astype(np.float32)) and np.array_equal(face, ref["face"]) and (face >= 0).all()
    v, f, _, _, sc = scene("icosphere_1280")
    rays = M.icosphere_seam_rays(v, f)
    ref = M.cast(v, f, rays)
    walk, brute = run(sc, to_dev(rays), 0), run(sc, to_dev(rays), 1)
    assert same_bits(walk, brute) and (walk[1] >= 0).all()                      # every vertex ray and every edge-midpoint ray hits
    assert np.array_equal(walk[1], ref["face"]) and np.array_equal(walk[0].view(np.uint32), ref["t_hit"].view(np.uint32))


@pytest.mark.parametrize("name", ["cube", "icosphere_1280", "body"])
def test_hit_faces(name):
    from youreditableavatar_amd import mesh_region
    v, f, rays, ref, sc = scene(name)
    r = to_dev(rays)
    ids = sc.cast_rays(r)["primitive_ids"]
    want = torch.zeros(len(f), dtype=torch.bool, device=DEV)
    want[torch.unique(ids[ids >= 0]).long()] = True
    for mode in (0, 1):
        hit = sc.hit_faces(r, mode=mode)
        assert hit.dtype == torch.bool and hit.device == torch.device(DEV) and torch.equal(hit, want)
    half = len(rays) // 2
    first = sc.hit_faces(r[:half])
    kept = first.clone()
    both = sc.hit_faces(r[half:], out=first)                                    # ORs into a previous camera's array
    assert both.data_ptr() == first.data_ptr() and torch.equal(both, want) and bool((both >= kept).all())
    with pytest.raises(RuntimeError, match="expected out as a contiguous bool tensor"):
        sc.hit_faces(r, out=torch.zeros(len(f) + 1, dtype=torch.bool, device=DEV))
    faces = sc._sdf._dev[1]
    region = mesh_region.refine_region(faces, sc.hit_faces(r), len(v), 1, 1)    # feeds refine_region as it is, on the device
    by_index = mesh_region.refine_region(faces, torch.unique(ids[ids >= 0]).long(), len(v), 1, 1)
    assert torch.equal(region.face_mask, by_index.face_mask) and torch.equal(region.vertex_mask, by_index.vertex_mask)


@pytest.mark.parametrize("name", ["cube", "two_cubes", "body"])
def test_occlusions_against_the_cast(name):
    v, f, rays, ref, sc = scene(name)
    r = to_dev(rays)
    t = sc.cast_rays(r)["t_hit"]
    ok = to_dev(~ref["flag"])
    for tnear, tfar in ((0.0, float("inf")), (-1.0, 0.75), (0.0, 1.0), (0.5, 1.5)):
        occ = sc.test_occlusions(r, tnear, tfar)
        assert torch.equal(occ, sc.test_occlusions(r, tnear, tfar, mode=1))
        inside = torch.isfinite(t) & (t >= tnear) & (t <= tfar)                 # (t_hit is rounded: a t within an ulp of a bound is not compared)
        near = torch.isfinite(t) & (((t - tnear).abs() <= 1e-6 * t.abs()) | ((t - tfar).abs() <= 1e-6 * t.abs()))
        if tnear <= 0.0:
            assert torch.equal(occ[ok & ~near], inside[ok & ~near])
        assert bool(occ[ok & inside & ~near].all())
    if name == "cube":                                                          # tfar just below and just above a known hit: this ray meets the cube at t = 2 and leaves at 3
        ray = torch.tensor([[0.25, 0.5, -2, 0, 0, 1]], device=DEV)
        below, above = float(np.nextafter(np.float32(2), np.float32(0))), float(np.nextafter(np.float32(2), np.float32(4)))
        for mode in (0, 1):
            got = [bool(sc.test_occlusions(ray, a, b, mode=mode)[0]) for a, b in ((0.0, below), (0.0, 2.0), (0.0, above), (above, 2.5), (above, 3.0))]
            assert got == [False, True, True, False, True]
        with pytest.raises(RuntimeError, match="tnear <= tfar"):
            sc.test_occlusions(ray, 1.0, 0.5)


def test_from_sdf_shares_the_tree():
    from youreditableavatar_amd.mesh_rays import RaycastingScene
    from youreditableavatar_amd.mesh_sdf import SDF
    v, f, rays, ref, sc = scene("body")
    sdf = SDF(to_dev(v), to_dev(f))
    shared = RaycastingScene.from_sdf(sdf)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(shared._sdf._dev, sdf._dev)) and shared.device == sdf.device
    r = to_dev(rays)
    assert same_bits(run(shared, r, 0), run(sc, r, 0))
    assert torch.isfinite(sdf(r[:64, :3])).all()                                # the SDF still answers from the same bytes


def test_call_shapes():
    from youreditableavatar_amd.mesh_rays import RaycastingScene
    v, f, rays, ref, sc = scene("cube")
    from_numpy = RaycastingScene()
    assert from_numpy.add_triangles(v.astype(np.float64), f.astype(np.int64)) == 0          # as the reference passes them
    assert from_numpy.device == torch.device("cuda", torch.cuda.current_device())
    out = from_numpy.cast_rays(rays[None].astype(np.float64))                   # numpy in, numpy out, the reference's [1, M, 6]
    assert all(isinstance(a, np.ndarray) for a in out.values()) and out["t_hit"].dtype == np.float32 and out["t_hit"].shape == (1, len(rays))
    ids = out["primitive_ids"]
    assert ids.dtype == np.uint32 and out["geometry_ids"].dtype == np.uint32 and RaycastingScene.INVALID_ID == 4294967295
    assert np.array_equal(ids < RaycastingScene.INVALID_ID, np.isfinite(out["t_hit"])) and (ids[0, -3:] == RaycastingScene.INVALID_ID).all()
    hit_set = set(ids[ids < RaycastingScene.INVALID_ID].tolist())               # the reference's loop
    on_device = sc.cast_rays(to_dev(rays))
    for k, a in on_device.items():
        assert isinstance(a, torch.Tensor) and a.device == torch.device(DEV) and not a.requires_grad, k
        assert np.array_equal(a.cpu().numpy().view(np.uint32), out[k][0].view(np.uint32)), k
    assert on_device["primitive_ids"].dtype == torch.int32 and on_device["geometry_ids"].dtype == torch.int32 and int(on_device["primitive_ids"].min()) == -1
    assert hit_set == set(torch.nonzero(sc.hit_faces(to_dev(rays)))[:, 0].tolist())
    occ = from_numpy.test_occlusions(rays)
    assert isinstance(occ, np.ndarray) and occ.dtype == np.bool_ and np.array_equal(occ, np.isfinite(out["t_hit"][0]))
    assert sc.cast_rays(torch.zeros(0, 6, device=DEV))["primitive_normals"].shape == (0, 3) and from_numpy.cast_rays(np.zeros((0, 6)))["t_hit"].shape == (0,)
    moving = to_dev(rays).requires_grad_()
    assert not sc.cast_rays(moving)["t_hit"].requires_grad                      # no autograd
    with pytest.raises(RuntimeError, match="no CPU path: rays must be on a HIP device"):
        sc.cast_rays(torch.tensor(rays))                                        # a CPU tensor next to a device mesh
    with pytest.raises(NotImplementedError, match="does not serve count_intersections"):
        sc.count_intersections(rays)
    with pytest.raises(RuntimeError, match="one mesh per scene"):
        sc.add_triangles(v, f)


def test_the_example_runs():
    import importlib.util
    import os
    from tests.util import ROOT
    spec = importlib.util.spec_from_file_location("back_project_rays", os.path.join(ROOT, "examples", "back_project_rays.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = example.run(subdivisions=5, W=128, H=128, device=DEV, log=lambda *a: None)       # (a coarser sphere's region does not survive refine_region(2, 5))
    assert out["hit"].any() and out["face_mask"].any() and out["vertex_mask"].sum() >= 3
