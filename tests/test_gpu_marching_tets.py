"""GPU: youreditableavatar_amd.marching_tets against what the reference's own ``_forward`` returned (tests/golden/ref_mt_fixture.npz: cases16, fan,
kuhn_8) and against the float64 restatement (tests/mt_ref.py: kuhn_32, the smallest grid with indices above 2^16 and several workgroups' worth
of tetrahedra in the scans).

Integers are exact.  Floats follow the project's rule: max |got - ref64| <= 4 eta with eta = max |ref32 - ref64| of the same restatement run in
float32; gradients add rel-L2 <= 4x ref32's and exact zeros on untouched rows (tests/mesh_grad_ref.py's ``check_bars``; the backward is a gather
in double, so there is no fixed-point term).  The gradient scenes keep every |sdf| on a crossing edge above 1e-6 cell (tests/test_mt_ref.py
asserts it), so nothing is left out.  kuhn_32's counts are constants taken from the float64 restatement."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_aa_ref as A
from tests import mesh_grad_ref as G
from tests import mt_ref as R

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
SCENES = ("cases16", "fan", "kuhn_8", "kuhn_32")
KUHN_32 = dict(valid=12632, verts=8260, faces=16516)


def _mt():
    import youreditableavatar_amd.marching_tets as mt
    return mt


def _dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def expected(name):
    """-> (integer outputs and float64 verts to compare with, float32 verts of the restatement)"""
    r64, r32 = R.reference(name)
    if name in R.FIXTURE_SCENES:                                             # the reference's own outputs where they are recorded
        fx = R.fixture()
        want = {k: fx[f"{name}.{k}"] for k in R.KEYS}
        want["interp_v"] = want["interp_v"].reshape(-1, 2)
        return want, r32["verts"]
    return r64, r32["verts"]


def run(name, idx=torch.int64, column=False, grad=False):
    s = R.scene(name)
    pos, sdf = _dev(s["pos"], grad), _dev(s["sdf"][:, None] if column else s["sdf"], grad)
    return _mt().marching_tets(pos, sdf, _dev(s["tet"]).to(idx)), pos, sdf


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
@pytest.mark.parametrize("column", [False, True])
def test_integers_are_exact_and_verts_within_four_eta(name, idx, column):
    want, v32 = expected(name)
    out, _, _ = run(name, idx, column)
    assert set(out) == set(R.KEYS)
    for k, dtype in (("valid_tets", torch.bool), ("interp_v", torch.int64), ("faces", torch.int64), ("face_to_tet_idx", torch.int64)):
        assert out[k].dtype == dtype and out[k].is_cuda and tuple(out[k].shape) == want[k].shape, (k, out[k].dtype, tuple(out[k].shape), want[k].shape)
        assert np.array_equal(_np(out[k]), want[k]), (name, k)
    got, v64 = _np(out["verts"]), want["verts"]
    assert got.dtype == np.float32 and got.shape == v64.shape
    assert np.array_equal(np.isnan(got), np.isnan(v64))                      # (fan: the vertices on the NaN corner's edges; nowhere else)
    live = ~np.isnan(v64)
    eta, err = float(np.abs(v32 - v64)[live].max()), float(np.abs(got - v64)[live].max())
    print(f"{name} verts: eta {eta:.3g} err {err:.3g}")
    assert err <= 4.0 * eta, (name, err, eta)
    if name == "kuhn_32":
        assert (int(_np(out["valid_tets"]).sum()), len(got), len(want["faces"])) == (KUHN_32["valid"], KUHN_32["verts"], KUHN_32["faces"])


def test_the_kuhn_32_mesh_is_closed_and_consistently_oriented():
    out, _, _ = run("kuhn_32")
    m = R.manifold_counts(_np(out["faces"]), len(out["verts"]))
    assert m == dict(directed_repeated=0, undirected_not_two=0, euler=2, unused_verts=0), m


# ---- gradients -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_grads(name, tag):
    """-> ((d_pos, d_sdf) in float64, the same evaluated in float32, the upstream), the restatement's autograd, read-only"""
    s, M = R.scene(name), len(R.reference(name)[0]["verts"])
    g = upstream(name, M, tag)
    res = []
    for f in (F64, F32):
        pos, sdf = torch.tensor(s["pos"]).to(f).requires_grad_(True), torch.tensor(s["sdf"]).to(f).requires_grad_(True)
        (R.marching_tets(pos, sdf, torch.tensor(s["tet"]))["verts"] * torch.tensor(g).to(f)).sum().backward()
        res.append((pos.grad.double().numpy(), sdf.grad.double().numpy()[:, None]))
    return res[0], res[1], g


def upstream(name, M, tag):
    iv = R.reference(name)[0]["interp_v"]
    g = np.zeros((M, 3), np.float32)
    if tag == "random":
        g[:] = np.random.default_rng(500 + M).uniform(-1.0, 1.0, (M, 3))
    elif tag in ("first", "last"):
        g[0 if tag == "first" else M - 1] = (1.0, -0.5, 0.25)
    else:                                                                    # "both_ends": the edges of a grid vertex that is the min end of some and the max end of others
        both = np.intersect1d(iv[:, 0], iv[:, 1])
        assert len(both) > 0
        v = both[len(both) // 2]
        rows = (iv == v).any(axis=1)
        assert (iv[rows, 0] == v).any() and (iv[rows, 1] == v).any()
        g[rows] = np.random.default_rng(7).uniform(-1.0, 1.0, (int(rows.sum()), 3))
    return g


@pytest.mark.parametrize("name,tag", [("kuhn_8", "random"), ("kuhn_32", "random"), ("kuhn_8", "first"), ("kuhn_8", "last"), ("kuhn_32", "last"), ("kuhn_8", "both_ends"),
                                      ("kuhn_32", "both_ends")])
@pytest.mark.parametrize("column", [False, True])
def test_gradients(name, tag, column):
    ref64, ref32, g = ref_grads(name, tag)
    out, pos, sdf = run(name, torch.int32 if column else torch.int64, column, grad=True)
    assert out["verts"].requires_grad and not any(out[k].requires_grad for k in R.KEYS[1:])
    out["verts"].backward(_dev(g))
    assert pos.grad.shape == pos.shape and sdf.grad.shape == sdf.shape and pos.grad.dtype == sdf.grad.dtype == torch.float32 and pos.grad.is_cuda
    G.check_bars(f"{name} {tag} dL_dpos", _np(pos.grad), ref64[0], ref32[0])
    G.check_bars(f"{name} {tag} dL_dsdf", _np(sdf.grad).reshape(-1, 1), ref64[1], ref32[1])
    touched = np.zeros(len(ref64[0]), bool)
    touched[R.reference(name)[0]["interp_v"][g.any(axis=1)].reshape(-1)] = True
    assert not _np(pos.grad)[~touched].any() and not _np(sdf.grad).reshape(-1)[~touched].any()


def test_a_gradient_is_computed_only_for_the_input_that_needs_one():
    s = R.scene("kuhn_8")
    ref64, ref32, g = ref_grads("kuhn_8", "random")
    for need_pos in (True, False):
        pos, sdf = _dev(s["pos"], need_pos), _dev(s["sdf"], not need_pos)
        _mt().marching_tets(pos, sdf, _dev(s["tet"]))["verts"].backward(_dev(g))
        mine, other = (pos, sdf) if need_pos else (sdf, pos)
        assert other.grad is None
        G.check_bars("one input", _np(mine.grad).reshape(len(s["pos"]), -1), ref64[0 if need_pos else 1], ref32[0 if need_pos else 1])
    with torch.no_grad():                                                    # the forward alone
        out = _mt().marching_tets(_dev(s["pos"], True), _dev(s["sdf"], True), _dev(s["tet"]))
    assert not out["verts"].requires_grad
    assert not _mt().marching_tets(_dev(s["pos"]), _dev(s["sdf"]), _dev(s["tet"]))["verts"].requires_grad


def test_two_runs_give_the_same_bits():
    _, _, g = ref_grads("kuhn_32", "random")
    runs = []
    for _ in range(2):
        out, pos, sdf = run("kuhn_32", grad=True)
        out["verts"].backward(_dev(g))
        runs.append([_np(out[k]) for k in R.KEYS] + [_np(pos.grad), _np(sdf.grad)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the edges of the domain -----------------------------------------------------------------------------------------------------------
def _assert_empty(out, F):
    assert [tuple(out[k].shape) for k in R.KEYS] == [(0, 3), (0, 3), (0,), (F,), (0, 2)]
    assert [out[k].dtype for k in R.KEYS] == [torch.float32, torch.int64, torch.int64, torch.bool, torch.int64]
    assert not out["valid_tets"].any()


@pytest.mark.parametrize("what", ["all_inside", "all_outside", "no_tets", "nothing"])
def test_empty_results_and_zero_gradients(what):
    s = R.scene("kuhn_8")
    N = 0 if what == "nothing" else len(s["pos"])
    F = 0 if what in ("no_tets", "nothing") else len(s["tet"])
    pos = _dev(s["pos"][:N], True)
    sdf = _dev(np.full(N, -1.0 if what == "all_outside" else 1.0, np.float32), True)
    out = _mt().marching_tets(pos, sdf, _dev(s["tet"][:F]))
    _assert_empty(out, F)
    (out["verts"].sum() * 2.0).backward()
    assert pos.grad.shape == pos.shape and sdf.grad.shape == sdf.shape and not pos.grad.any() and not sdf.grad.any()


def test_an_index_out_of_range_raises_and_the_device_stays_usable():
    """an argument check: the flag travels with the counts, the kernels never read through the index"""
    s = R.scene("kuhn_8")
    N = len(s["pos"])
    for bad, idx in ((N, torch.int64), (-1, torch.int32), (1 << 40, torch.int64), (-(1 << 33), torch.int64)):
        tet = s["tet"].copy()
        tet[len(tet) // 2, 2] = bad
        with pytest.raises(RuntimeError, match=r"outside \[0, 729\)"):
            _mt().marching_tets(_dev(s["pos"]), _dev(s["sdf"]), _dev(tet).to(idx) if idx == torch.int64 else _dev(tet.astype(np.int32)))
    with pytest.raises(RuntimeError, match="outside"):                     # no vertices at all, but tetrahedra
        _mt().marching_tets(_dev(s["pos"][:0]), _dev(s["sdf"][:0]), _dev(s["tet"]))
    want, _ = expected("kuhn_8")
    out, _, _ = run("kuhn_8")
    assert np.array_equal(_np(out["faces"]), want["faces"])


def test_the_batched_wrapper_agrees():
    s = R.scene("kuhn_8")
    out, _, _ = run("kuhn_8")
    pos, sdf, tet = _dev(s["pos"]), _dev(s["sdf"]), _dev(s["tet"])
    for sd in (sdf[None], sdf[None, :, None]):
        res = _mt().marching_tetrahedra(pos[None], tet, sd)
        assert len(res) == 2 and all(isinstance(r, list) and len(r) == 1 for r in res)
        assert torch.equal(res[0][0], out["verts"]) and torch.equal(res[1][0], out["faces"])
        res = _mt().marching_tetrahedra(torch.stack([pos, pos]), tet, torch.cat([sd, -sd]), return_tet_idx=True)
        assert len(res) == 3 and all(len(r) == 2 for r in res)
        assert torch.equal(res[0][0], out["verts"]) and torch.equal(res[1][0], out["faces"]) and torch.equal(res[2][0], out["face_to_tet_idx"])
        assert len(res[0][1]) == len(out["verts"])                           # the negated field crosses the same edges


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
CAMERA = np.array([[1.7, 0.0, 0.0, -0.85], [0.0, 1.7, 0.0, -0.85], [0.0, 0.0, 0.8, -0.4], [0.0, 0.0, 0.4, 0.8]], np.float32)     # w = 1 + 0.4 (z - 1/2)


def _clip(verts, cam):
    return torch.cat([verts, torch.ones_like(verts[:, :1])], 1) @ cam.T


def test_the_chain_into_the_mesh_rasterizer():
    """marching_tets -> rasterize / interpolate / antialias at 64^2 -> a mask and colour loss; d loss / d sdf against the restatement's chain on
    the device's integer decisions, within the bar tests/test_gpu_mesh_grad.py uses for its own chain"""
    import youreditableavatar_amd.mesh_raster_grad as dr
    s, H, W = R.scene("kuhn_8"), 64, 64
    out, pos, sdf = run("kuhn_8", grad=True)
    verts, tri = out["verts"], out["faces"].int()
    clip = _clip(verts, _dev(CAMERA))
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), clip, tri, (H, W))
    host_rast, host_clip, host_tri = _np(rast[0]), _np(clip), _np(tri)
    V = len(host_clip)
    amb, n_cov = G.uv_ambiguous(host_clip, host_tri, host_rast)
    assert n_cov > 500 and amb.sum() <= 0.02 * n_cov
    keep = (~amb).astype(np.float32).reshape(H, W, 1)                        # pixels at a clamp bound carry no colour (a fixed weight, both sides)
    g_c, g_o = G.upstream("kuhn_8", (H, W, 3), "mt_chain_c"), G.upstream("kuhn_8", (H, W, 1), "mt_chain_o")
    col, _ = dr.interpolate(verts, rast, tri)
    mask = (rast[..., 3:] > 0).float()
    img = col * mask * _dev(keep)[None]
    loss = (dr.antialias(img, rast, clip, tri) * _dev(g_c)[None]).sum() + (dr.antialias(mask, rast, clip, tri) * _dev(g_o)[None]).sum()
    loss.backward()
    got = _np(sdf.grad)
    assert np.isfinite(got).all() and np.isfinite(_np(pos.grad)).all()
    touched = np.zeros(len(got), bool)
    touched[_np(out["interp_v"]).reshape(-1)] = True
    assert not got[~touched].any() and got[touched].any()

    pix, vid = G.covered(host_rast, host_tri, V)
    pr = G.aa_pairs(host_rast, host_clip, host_tri, A.topology(host_tri, V))
    assert len(pr["R"]) > 50
    ref = {}
    for f in (F64, F32):
        p, sd = torch.tensor(s["pos"]).to(f).requires_grad_(True), torch.tensor(s["sdf"]).to(f).requires_grad_(True)
        o = R.marching_tets(p, sd, torch.tensor(s["tet"]))
        assert np.array_equal(o["faces"].numpy(), host_tri)
        v = o["verts"]
        c = _clip(v, torch.tensor(CAMERA).to(f))
        vt = torch.from_numpy(vid).reshape(-1)
        u_, v_, _, _ = G.uv_torch(c[vt].reshape(-1, 3, 4), torch.from_numpy(pix % W), torch.from_numpy(pix // W), W, H)
        colr = torch.zeros((H * W, 3), dtype=f).index_add(0, torch.from_numpy(pix), G.interpolate_torch(v[vt].reshape(-1, 3, 3), torch.stack([u_, v_], 1)))
        m = torch.zeros((H * W, 1), dtype=f)
        m[pix] = 1.0
        im = colr * m * G._t(keep.reshape(-1, 1), f)
        PA, PB = c[torch.from_numpy(pr["va"])], c[torch.from_numpy(pr["vb"])]
        (( G.aa_torch(im, PA, PB, pr, W, H) * G._t(g_c.reshape(-1, 3), f)).sum() + (G.aa_torch(m, PA, PB, pr, W, H) * G._t(g_o.reshape(-1, 1), f)).sum()).backward()
        ref[f] = (p.grad.double().numpy(), sd.grad.double().numpy()[:, None])
    G.check_bars("kuhn_8 chain dL_dsdf", got.reshape(-1, 1), ref[F64][1], ref[F32][1])
    G.check_bars("kuhn_8 chain dL_dpos", _np(pos.grad), ref[F64][0], ref[F32][0])


def test_the_example_lowers_its_loss_on_a_mesh_that_changes_size():
    import importlib.util
    import os
    from tests.util import ROOT
    spec = importlib.util.spec_from_file_location("fit_sdf_silhouette", os.path.join(ROOT, "examples", "fit_sdf_silhouette.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.fit(grid=12, resolution=64, steps=30, verbose=False)
    print(f"fit_sdf_silhouette, 12^3 cubes at 64^2, 30 steps: loss {res['first_loss']:.5f} -> {res['last_loss']:.5f} (factor {res['first_loss'] / res['last_loss']:.2f}), "
          f"{res['mesh_sizes_seen']} mesh sizes")
    assert res["last_loss"] < res["first_loss"]
    assert res["mesh_sizes_seen"] > 1
