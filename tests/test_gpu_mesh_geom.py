"""GPU: youreditableavatar_amd.mesh_geom against what the reference's own functions returned (tests/golden/ref_mesh_geom_fixture.npz: cases16, fan,
kuhn_8, traps) and against the float64 restatement (tests/mesh_geom_ref.py: kuhn_32 and kuhn_32_small, whose scans span several workgroups, and
umbrella, whose apex has a run longer than a wave).

Integers are exact.  Floats follow the project's rule: max |got - ref64| <= 4 eta with eta = max |ref32 - ref64| of the same restatement run in
float32; gradients add rel-L2 <= 4x ref32's and exact zeros on the rows the reference leaves at zero (tests/mesh_grad_ref.py's ``check_bars``; the
backward is a gather in double, so there is no fixed-point term).  Non-finite rows (fan) are compared row-wise.  kuhn_32_small's rows within a
factor 2 of the 1e-20 threshold take no part (tests/test_mesh_geom_ref.py bounds their number), and carry no upstream."""
import numpy as np
import pytest
import torch

from tests import mesh_geom_ref as R

pytestmark = pytest.mark.gpu
SCALARS = ("consistency", "consistency_of_normals", "laplacian")


def _mg():
    import youreditableavatar_amd.mesh_geom as mg
    return mg


def _dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def mesh(name, idx=torch.int64, grad=False):
    m = R.scene(name)
    return _dev(m["v_pos"], grad), _dev(m["faces"]).to(idx)


def want_edges(name):
    return R.fixture()[f"{name}.edges"] if name in R.FIXTURE_SCENES else R.edges_of(torch.tensor(R.scene(name)["faces"])).numpy()


def run_scalar(what, name, topo, grad=True):
    """-> (the value, the leaf) of one of SCALARS on the device"""
    mg = _mg()
    v, f = mesh(name, grad=grad and what != "consistency")
    if what == "consistency":
        leaf = _dev(R.reference(name, "normals")[1][0].astype(np.float32), grad)
        return mg.normal_consistency(leaf, topo if topo is not None else mg.mesh_topology(f, len(v))), leaf
    if what == "consistency_of_normals":
        return mg.mesh_normal_consistency(v, f, topo), v
    return mg.laplacian(v, topo if topo is not None else mg.mesh_topology(f, len(v))), v


# ---- the topology ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SCENES)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_edges_and_runs_are_exact(name, idx):
    v, f = mesh(name, idx)
    topo = _mg().mesh_topology(f, len(v))
    want, faces, V = want_edges(name), R.scene(name)["faces"], len(v)
    assert topo.edges.dtype == torch.int64 and topo.edges.is_cuda and tuple(topo.edges.shape) == want.shape and topo.num_edges == len(want)
    assert np.array_equal(_np(topo.edges), want)
    if name == "traps":
        assert (want[:, 0] == want[:, 1]).sum() == 4                            # the pairs (i, i) are kept
    words = lambda t: _np(t).view(np.uint32).astype(np.int64)
    flat = faces.reshape(-1)
    assert np.array_equal(words(topo.inc), np.argsort(flat, kind="stable"))     # each vertex's run in ascending 3 * face + corner
    assert np.array_equal(words(topo.inc_end)[:V], np.cumsum(np.bincount(flat, minlength=V)))
    assert np.array_equal(words(topo.edge_end)[:V], np.cumsum(np.bincount(want[:, 0], minlength=V)))
    assert np.array_equal(words(topo.max_end)[:V], np.cumsum(np.bincount(want[:, 1], minlength=V)))
    assert np.array_equal(words(topo.max_list), np.argsort(want[:, 1], kind="stable"))
    bare = _mg().mesh_topology(f, len(v), edges=False)
    assert bare.edges is None and torch.equal(bare.inc, topo.inc) and torch.equal(bare.inc_end, topo.inc_end)


# ---- values and gradients --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SCENES)
@pytest.mark.parametrize("tag", ["random", "one_row"])
def test_vertex_normals_and_their_gradient(name, tag):
    (v64, g64), (v32, g32) = R.reference(name, "normals", tag)
    v, f = mesh(name, torch.int32 if tag == "one_row" else torch.int64, grad=True)
    out = _mg().vertex_normals(v, f)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == v64.shape and out.requires_grad
    out.backward(_dev(R.upstream(name, tag)))
    skip = R.left_out(name)
    R.compare(f"{name} normals", _np(out), v64, v32, skip)
    R.compare(f"{name} {tag} normals dL_dv_pos", _np(v.grad), g64, g32, skip)
    sq, _ = R.row_figures(name)
    default = sq <= R.NORMAL_EPS
    if name == "kuhn_32_small":
        assert int(default.sum()) == R.KUHN_32_SMALL_DEFAULT_ROWS and int(skip.sum()) <= 2
    assert np.array_equal(_np(out)[default], np.tile(np.float32([0, 0, 1]), (int(default.sum()), 1)))
    if name in R.FIXTURE_SCENES and tag == "random":                            # the reference's own numbers, both of its functions
        fx = R.fixture()
        for key in ("compute_normal", "v_nrm"):
            R.compare(f"{name} {key}", _np(out), fx[f"{name}.{key}"], v32)
        R.compare(f"{name} compute_normal gradient", _np(v.grad), fx[f"{name}.compute_normal.grad"], g32)


@pytest.mark.parametrize("name", R.SCENES)
@pytest.mark.parametrize("what", SCALARS)
def test_the_losses_and_their_gradients(name, what):
    (v64, g64), (v32, g32) = R.reference(name, what)
    out, leaf = run_scalar(what, name, None)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.is_cuda and out.requires_grad
    (out * float(R.SCALAR_UPSTREAM)).backward()
    R.compare(f"{name} {what}", _np(out), v64, v32)
    by_rule = R.rules_zero_rows(name) if what == "consistency_of_normals" else None
    R.compare(f"{name} {what} gradient", _np(leaf.grad), g64, g32, exact_zero=by_rule)
    key = dict(consistency_of_normals="normal_consistency", laplacian="laplacian").get(what)
    if name in R.FIXTURE_SCENES and key:
        fx = R.fixture()
        R.compare(f"{name} {key} (fixture)", _np(out), fx[f"{name}.{key}"], v32)
        R.compare(f"{name} {key} gradient (fixture)", _np(leaf.grad), fx[f"{name}.{key}.grad"], g32, exact_zero=by_rule)


# ---- properties ------------------------------------------------------------------------------------------------------------------------
def _everything(name, topo_given):
    """every output and gradient of the four calls as bytes, with one topology for all calls or with ``topology=None`` where that is allowed"""
    mg = _mg()
    v, f = mesh(name, grad=True)
    topo = mg.mesh_topology(f, len(v))
    n = mg.vertex_normals(v, f, topo if topo_given else None)
    n.backward(_dev(R.upstream(name, "random")))
    res = [_np(topo.edges), _np(topo.inc), _np(topo.max_list), _np(n), _np(v.grad)]
    for what in SCALARS:
        out, leaf = run_scalar(what, name, topo if topo_given or what != "consistency_of_normals" else None)
        out.backward()
        res += [_np(out), _np(leaf.grad)]
    return [np.atleast_1d(a).view(np.uint8) for a in res]


@pytest.mark.parametrize("name", ["kuhn_32", "umbrella"])
def test_two_runs_give_the_same_bits_and_a_reused_topology_changes_nothing(name):
    first = _everything(name, True)
    for other in (_everything(name, True), _everything(name, False)):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)


def test_a_topology_serves_three_calls_and_parameters_are_leaves():
    mg = _mg()
    m = R.scene("kuhn_8")
    p = torch.nn.Parameter(_dev(m["v_pos"]))
    f = _dev(m["faces"])
    topo = mg.mesh_topology(f, len(p))
    loss = mg.normal_consistency(mg.vertex_normals(p, f, topo), topo) + 0.5 * mg.laplacian(p, topo) + mg.vertex_normals(p, f, topo)[:, 2].mean()
    loss.backward()
    assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() and p.grad.any()
    q = torch.nn.Parameter(_dev(m["v_pos"]))
    (mg.mesh_normal_consistency(q, f) + 0.5 * mg.laplacian(q, mg.mesh_topology(f, len(q))) + mg.vertex_normals(q, f)[:, 2].mean()).backward()
    assert torch.equal(p.grad, q.grad)


def test_no_gradient_wanted_is_the_forward_alone():
    mg = _mg()
    v, f = mesh("kuhn_8", grad=True)
    topo = mg.mesh_topology(f, len(v))
    with torch.no_grad():
        outs = [mg.vertex_normals(v, f, topo), mg.normal_consistency(v, topo), mg.laplacian(v, topo), mg.mesh_normal_consistency(v, f, topo)]
    assert not any(o.requires_grad for o in outs)
    d = v.detach()
    plain = [mg.vertex_normals(d, f, topo), mg.normal_consistency(d, topo), mg.laplacian(d, topo), mg.mesh_normal_consistency(d, f, topo)]
    assert not any(o.requires_grad for o in plain) and all(torch.equal(a, b) for a, b in zip(outs, plain))


def test_an_index_out_of_range_raises_and_the_device_stays_usable():
    """an argument check: the flag travels with the edge count, the kernels never read through the index"""
    mg = _mg()
    m = R.scene("kuhn_8")
    V = len(m["v_pos"])
    for bad, idx in ((V, torch.int64), (-1, torch.int32), (1 << 40, torch.int64), (-(1 << 33), torch.int64)):
        faces = m["faces"].copy()
        faces[len(faces) // 2, 1] = bad
        f = _dev(faces) if idx == torch.int64 else _dev(faces.astype(np.int32))
        with pytest.raises(RuntimeError, match=rf"outside \[0, {V}\)"):
            mg.mesh_topology(f, V)
        with pytest.raises(RuntimeError, match="outside"):
            mg.vertex_normals(_dev(m["v_pos"]), f)
    with pytest.raises(RuntimeError, match="outside"):                         # no vertices at all, but faces
        mg.mesh_topology(_dev(m["faces"]), 0)
    assert np.array_equal(_np(mg.mesh_topology(_dev(m["faces"]), V).edges), want_edges("kuhn_8"))


@pytest.mark.parametrize("V,F", [(0, 0), (7, 0)])
def test_empty_inputs(V, F):
    mg = _mg()
    v = torch.zeros((V, 3), device="cuda").requires_grad_(True)
    f = torch.zeros((F, 3), dtype=torch.int64, device="cuda")
    topo = mg.mesh_topology(f, V)
    assert tuple(topo.edges.shape) == (0, 2) and topo.edges.dtype == torch.int64 and topo.num_edges == 0
    n = mg.vertex_normals(v, f, topo)
    assert tuple(n.shape) == (V, 3) and n.dtype == torch.float32 and torch.equal(n, torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(V, 3))
    nc, lap = mg.normal_consistency(n, topo), mg.laplacian(v, topo)
    assert nc.dim() == 0 and lap.dim() == 0 and torch.isnan(nc)                # the mean of nothing
    assert torch.isnan(lap) if V == 0 else float(lap.detach()) == 0.0
    (n.sum() + (lap if V else 0.0)).backward()
    assert v.grad.shape == v.shape and not v.grad.any()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
CAMERA = np.array([[1.7, 0.0, 0.0, -0.85], [0.0, 1.7, 0.0, -0.85], [0.0, 0.0, 0.8, -0.4], [0.0, 0.0, 0.4, 0.8]], np.float32)     # w = 1 + 0.4 (z - 1/2)
LAMBDA_NC = 2.0


def _clip(verts, cam):
    return torch.cat([verts, torch.ones_like(verts[:, :1])], 1) @ cam.T


def test_the_chain_from_the_sdf_to_a_normal_map_and_the_consistency_loss():
    """marching_tets -> vertex_normals -> rasterize / interpolate at 64^2 -> a normal-map loss + mesh_normal_consistency; d loss / d sdf and d pos
    against the restatements' chain on the device's integer decisions.  Float32 framework kernels sit between the calls, so the bar is 4 eta of
    the same chain in float32."""
    import youreditableavatar_amd.marching_tets as mt
    import youreditableavatar_amd.mesh_raster_grad as dr
    from tests import mesh_grad_ref as G
    from tests import mt_ref as MT
    mg = _mg()
    s, H, W = MT.scene("kuhn_8"), 64, 64
    pos, sdf = _dev(s["pos"], True), _dev(s["sdf"], True)
    out = mt.marching_tets(pos, sdf, _dev(s["tet"]))
    verts, tri = out["verts"], out["faces"].int()
    topo = mg.mesh_topology(out["faces"], len(verts))
    nrm = mg.vertex_normals(verts, out["faces"], topo)
    clip = _clip(verts, _dev(CAMERA))
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), clip, tri, (H, W))
    host_rast, host_clip, host_tri = _np(rast[0]), _np(clip), _np(tri)
    V = len(host_clip)
    amb, n_cov = G.uv_ambiguous(host_clip, host_tri, host_rast)
    assert n_cov > 500 and amb.sum() <= 0.02 * n_cov
    keep = (~amb).astype(np.float32).reshape(H, W, 1)                        # pixels at a clamp bound carry no colour (a fixed weight, both sides)
    g_c = G.upstream("kuhn_8", (H, W, 3), "mg_chain_c")
    col, _ = dr.interpolate(nrm, rast, tri)
    loss = (col * _dev(keep)[None] * _dev(g_c)[None]).sum() + LAMBDA_NC * mg.normal_consistency(nrm, topo)
    loss.backward()
    got_sdf, got_pos = _np(sdf.grad), _np(pos.grad)
    assert np.isfinite(got_sdf).all() and np.isfinite(got_pos).all() and got_sdf.any()

    pix, vid = G.covered(host_rast, host_tri, V)
    ref = {}
    for f in (R.F64, R.F32):
        p, sd = torch.tensor(s["pos"]).to(f).requires_grad_(True), torch.tensor(s["sdf"]).to(f).requires_grad_(True)
        o = MT.marching_tets(p, sd, torch.tensor(s["tet"]))
        assert np.array_equal(o["faces"].numpy(), host_tri)
        v = o["verts"]
        n = R.vertex_normals(v, o["faces"])
        c = _clip(v, torch.tensor(CAMERA).to(f))
        vt = torch.from_numpy(vid).reshape(-1)
        u_, v_, _, _ = G.uv_torch(c[vt].reshape(-1, 3, 4), torch.from_numpy(pix % W), torch.from_numpy(pix // W), W, H)
        colr = torch.zeros((H * W, 3), dtype=f).index_add(0, torch.from_numpy(pix), G.interpolate_torch(n[vt].reshape(-1, 3, 3), torch.stack([u_, v_], 1)))
        total = (colr * G._t(keep.reshape(-1, 1), f) * G._t(g_c.reshape(-1, 3), f)).sum() + LAMBDA_NC * R.normal_consistency(n, R.edges_of(o["faces"]))
        total.backward()
        ref[f] = (float(total), p.grad.double().numpy(), sd.grad.double().numpy()[:, None])
    print(f"kuhn_8 chain loss: device {float(loss):.9g} float64 {ref[R.F64][0]:.9g} float32 {ref[R.F32][0]:.9g}")
    G.check_bars("kuhn_8 normals chain dL_dsdf", got_sdf.reshape(-1, 1), ref[R.F64][2], ref[R.F32][2])
    G.check_bars("kuhn_8 normals chain dL_dpos", got_pos, ref[R.F64][1], ref[R.F32][1])


def test_the_example_lowers_its_loss():
    import importlib.util
    import os
    from tests.util import ROOT
    spec = importlib.util.spec_from_file_location("fit_sdf_normals", os.path.join(ROOT, "examples", "fit_sdf_normals.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.fit(grid=12, resolution=64, steps=30, verbose=False)
    print(f"fit_sdf_normals, 12^3 cubes at 64^2, 30 steps: loss {res['first_loss']:.5f} -> {res['last_loss']:.5f} (factor {res['first_loss'] / res['last_loss']:.2f}), "
          f"normal consistency {res['first_consistency']:.5f} -> {res['last_consistency']:.5f}, {res['mesh_sizes_seen']} mesh sizes")
    assert res["last_loss"] < res["first_loss"]
    assert res["mesh_sizes_seen"] > 1
