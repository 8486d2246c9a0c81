"""GPU: the mesh signed distance (youreditableavatar_amd.mesh_sdf, csrc/tgs_mesh_sdf.hip) against the float64 restatement (tests/mesh_sdf_ref.py)
under the four bars of ``mesh_sdf_ref.check_bars``, the tree walk against the walk over every face bit for bit, two runs bit for bit, the launch
shapes around a wave, and the module's call shapes.  The body mesh and its points come from tests/golden/ref_mesh_sdf_fixture.npz."""
import numpy as np
import pytest
import torch

from tests import mesh_sdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def scene(name):
    """-> (vertices, faces, points, the restatement's outputs, the SDF on the device), computed once per scene"""
    from youreditableavatar_amd.mesh_sdf import SDF
    if name not in _cache:
        if name == "body":
            v, f, pts, ref, _ = R.load_fixture()
        else:
            v, f = R.SCENES[name]()
            pts = R.scene_points(v)
            ref = R.query(v, f, pts)
        _cache[name] = (v, f, pts, ref, SDF(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)))
    return _cache[name]


def run(sdf, points, mode):
    """-> (sdf, face, closest, inside) as numpy arrays"""
    s, f, c = sdf.closest(points, mode=mode)
    s2, i = sdf(points, mode=mode), sdf.contains(points, mode=mode)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32))               # the same bits whichever outputs are asked for
    return s.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy(), i.cpu().numpy()


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(R.SCENES) + ["body"])
def test_scene_against_the_restatement_and_mode_0_against_mode_1(name):
    v, f, pts, ref, sdf = scene(name)
    assert sdf.device == torch.device(DEV)
    p = torch.from_numpy(pts).to(DEV)
    walk, brute = run(sdf, p, 0), run(sdf, p, 1)
    assert same_bits(walk, brute)                                               # equal bits of sdf and closest, equal face and inside
    assert same_bits(walk, run(sdf, p, 0)) and same_bits(brute, run(sdf, p, 1))  # two runs give equal bits
    R.check_bars(v, f, pts, ref, *walk, what=name)
    bad = ~np.isfinite(pts).all(axis=1)                                         # the NaN point and the infinite points: NaN, -1, False, and the call returned
    if name != "body":
        assert bad.sum() == 3 and np.isnan(walk[0][bad]).all() and (walk[1][bad] == -1).all() and not walk[3][bad].any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("name", ["body", "cube"])
def test_launch_shapes(name, n):
    v, f, pts, ref, sdf = scene(name)
    if name == "cube":                                                          # 4 097 points from 411: the scene's points over and over
        take = np.arange(n) % len(pts)
        pts, ref = pts[take], {k: a[take] for k, a in ref.items()}
    else:
        pts, ref = pts[:n], {k: a[:n] for k, a in ref.items()}
    p = torch.from_numpy(pts).to(DEV)
    walk, brute = run(sdf, p, 0), run(sdf, p, 1)
    assert walk[0].shape == (n,) and walk[1].shape == (n,) and walk[2].shape == (n, 3) and walk[3].shape == (n,) and walk[3].dtype == np.bool_
    assert same_bits(walk, brute)
    if n:
        R.check_bars(v, f, pts, ref, *walk, what=f"{name} N={n}")


def test_call_shapes():
    from youreditableavatar_amd.mesh_sdf import SDF
    v, f, pts, ref, sdf = scene("cube")
    from_numpy = SDF(v.astype(np.float64), f.astype(np.int64))                  # as the reference passes them: trimesh's float64 vertices and int64 faces
    assert from_numpy.device == torch.device("cuda", torch.cuda.current_device())
    out = from_numpy(pts.astype(np.float64))                                    # numpy in, numpy out: float32, as pysdf answers
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (len(pts),)
    on_device = sdf(torch.from_numpy(pts).to(DEV))
    assert isinstance(on_device, torch.Tensor) and on_device.device == torch.device(DEV) and on_device.dtype == torch.float32 and not on_device.requires_grad
    assert np.array_equal(out.view(np.uint32), on_device.cpu().numpy().view(np.uint32))
    inside = from_numpy.contains(pts)
    assert isinstance(inside, np.ndarray) and inside.dtype == np.bool_ and np.array_equal(inside[~ref["flag"]], ref["inside"][~ref["flag"]])
    s, face, closest = from_numpy.closest(pts)
    assert all(isinstance(a, np.ndarray) for a in (s, face, closest)) and face.dtype == np.int32 and closest.shape == (len(pts), 3)
    assert np.array_equal(s.view(np.uint32), out.view(np.uint32))
    t = sdf.contains(torch.from_numpy(pts).to(DEV))
    assert t.dtype == torch.bool and t.is_cuda
    assert isinstance(sdf.vertices, np.ndarray) and np.array_equal(sdf.vertices, v) and np.array_equal(sdf.faces, f)
    strided = torch.from_numpy(np.concatenate([pts, pts], axis=1)).to(DEV)[:, 3:]  # a view that is not contiguous
    assert torch.equal(sdf(strided).view(torch.int32), on_device.view(torch.int32))
    assert sdf(torch.zeros(0, 3, device=DEV)).shape == (0,) and from_numpy(np.zeros((0, 3))).shape == (0,)
    with pytest.raises(RuntimeError, match="robust=False"):
        SDF(v, f, robust=False)
    with pytest.raises(RuntimeError, match="does not serve nn"):
        sdf.nn(pts)
    with pytest.raises(RuntimeError, match="no CPU path: points must be on a HIP device"):
        sdf(torch.from_numpy(pts))                                              # a CPU tensor next to a device mesh
    with pytest.raises(RuntimeError, match=r"outside \[0, V\)"):
        SDF(torch.from_numpy(v).to(DEV), torch.from_numpy(f + 1).to(DEV))


def test_the_chain_to_the_field_and_back():
    """SDF -> SdfField -> mse -> backward, as one iteration of the shape initialisation runs it, on 4 096 points"""
    from youreditableavatar_amd import hashgrid
    v, f, _, _, sdf = scene("body")
    torch.manual_seed(0)
    config = dict(otype="HashGrid", n_levels=8, n_features_per_level=2, log2_hashmap_size=14, base_resolution=4, per_level_scale=1.5)
    encoding = hashgrid.HashGrid(3, config)
    mlp = torch.nn.Sequential(torch.nn.Linear(encoding.n_output_dims, 64, bias=False), torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 1, bias=False))
    field = hashgrid.SdfField(encoding, mlp, bbox=[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], bias=0.0).to(DEV)
    points = torch.rand(4096, 3, device=DEV) * 2.0 - 1.0
    target = -sdf(points)[..., None]                                            # the reference's sign: negative inside
    assert target.shape == (4096, 1) and not target.requires_grad and torch.isfinite(target).all() and (target < 0).any() and (target > 0).any()
    loss = torch.nn.functional.mse_loss(field(points), target)
    loss.backward()
    assert torch.isfinite(loss)
    for p in field.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any()
