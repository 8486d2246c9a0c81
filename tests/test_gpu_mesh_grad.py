"""GPU: youreditableavatar_amd.mesh_raster_grad (csrc/tgs_mesh_grad.hip) against the rules as tests/mesh_grad_ref.py restates them.

Bars, per gradient tensor (tests/mesh_grad_ref.py ``check_bars``; all from the restatement alone): max |got - ref64| <= 4 max |ref32 - ref64|
plus the header's fixed-point term n 2^(e-35) (n, B of the reference's own per-pixel contributions); rel-L2 against ref64 no larger than 4x
ref32's; where eta = 0 equality; rows the reference leaves at zero are exactly zero.  The factor 4 is the forward tests' margin for a
different summation order.  interpolate and antialias take the CPU reference's rast (uploaded); rasterize's backward takes the device's own
rast, and the reference is evaluated on the IDs it holds.  Pixels at a clamp bound of u, v (tests/mesh_grad_ref.py ``uv_ambiguous``) get a
zero upstream; no output is excluded.  eta and the kernels' errors per scene are in INTEGRATION.md 4l."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mesh_aa_ref as A
from tests import mesh_grad_ref as G
from tests.util import ROOT

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def _dr():
    import youreditableavatar_amd.mesh_raster_grad as dr
    return dr


def _dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)         # (a copy: the cached arrays are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def attrs(name, C):
    s = G.scene(name)
    return np.random.default_rng(sum(ord(ch) for ch in name) * 4 + C).uniform(-1.0, 1.0, (len(s["pos"]), C)).astype(np.float32)


# ---- one image through each call: -> the gradients as numpy arrays ---------------------------------------------------------------------
def run_interpolate(attr, rast, tri, g):
    a, r = _dev(attr, True), _dev(rast, True)
    out, none = _dr().interpolate(a, r[None], _dev(tri))
    assert none is None and out.shape == (1,) + g.shape
    out.backward(_dev(g)[None])
    assert a.grad.dtype == torch.float32 and a.grad.is_cuda and r.grad.dtype == torch.float32 and r.grad.shape == r.shape
    return _np(a.grad), _np(r.grad)


@functools.lru_cache(maxsize=None)
def device_rast(name):
    """the device's own rast of the scene: float32 [H,W,4], read-only"""
    s = G.scene(name)
    rast, _ = _dr().rasterize(_dr().RasterizeCudaContext(), _dev(s["pos"]), _dev(s["tri"]), (s["H"], s["W"]))
    a = _np(rast[0])
    a.setflags(write=False)
    return a


def run_rasterize(name, g):
    s = G.scene(name)
    p = _dev(s["pos"], True)
    rast, none = _dr().rasterize(_dr().RasterizeGLContext(), p, _dev(s["tri"]), (s["H"], s["W"]), grad_db=True)
    assert none is None and np.array_equal(_np(rast[0]).view(np.uint32), device_rast(name).view(np.uint32))
    rast.backward(_dev(g)[None])
    assert p.grad.dtype == torch.float32 and p.grad.is_cuda and p.grad.shape == p.shape
    return _np(p.grad)


def run_antialias(name, color, g, boost=1.0, topology=True):
    s = G.scene(name)
    c, p, tri = _dev(color, True), _dev(s["pos"], True), _dev(s["tri"])
    topo = _dr().antialias_construct_topology_hash(tri, num_vertices=len(s["pos"])) if topology else None
    out = _dr().antialias(c[None], _dev(G.scene_rast(name))[None], p, tri, topology_hash=topo, pos_gradient_boost=boost)
    out.backward(_dev(g)[None])
    return _np(c.grad), _np(p.grad), _np(out[0])


def uv_upstream(name, tag="rast"):
    """a random upstream for rast [H,W,4] (z/w and ID channels included: they are ignored), zero on the pixels at a clamp bound"""
    s = G.scene(name)
    g = G.upstream(name, (s["H"], s["W"], 4), tag)
    amb, n = G.uv_ambiguous(s["pos"], s["tri"], device_rast(name))
    g[amb] = 0.0
    return g, int(amb.sum()), n


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_256", "flaps_64x48"])
@pytest.mark.parametrize("grad", [False, True])
def test_forward_is_bit_equal_to_the_forward_only_modules(name, grad):
    import youreditableavatar_amd.mesh_raster_aa as fwd
    dr, s, C = _dr(), G.scene(name), 3
    tri = _dev(s["tri"])
    want_rast, _ = fwd.rasterize(None, _dev(s["pos"]), tri, (s["H"], s["W"]))
    want_attr, _ = fwd.interpolate(_dev(attrs(name, C)), want_rast, tri)
    want_out = fwd.antialias(want_attr, want_rast, _dev(s["pos"]), tri)
    pos, attr = _dev(s["pos"], grad), _dev(attrs(name, C), grad)
    rast, none = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, (s["H"], s["W"]))
    out_attr, none2 = dr.interpolate(attr, rast, tri, rast_db=None, diff_attrs=None)
    out = dr.antialias(out_attr, rast, pos, tri)
    assert none is None and none2 is None
    for got, want in ((rast, want_rast), (out_attr, want_attr), (out, want_out)):
        assert got.requires_grad == grad and (got.grad_fn is not None) == grad
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32))
    with torch.no_grad():                                                     # no graph wanted: the forward-only calls, whatever the inputs require
        assert torch.equal(dr.rasterize(None, pos, tri, (s["H"], s["W"]))[0].view(torch.int32), want_rast.view(torch.int32))


# ---- against the reference -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interpolate_case(name, C):
    s = G.scene(name)
    attr, rast, g = attrs(name, C), G.scene_rast(name), G.upstream(name, (s["H"], s["W"], C), "interp")
    return attr, g, G.interpolate_grads(F64, attr, rast, s["tri"], g), G.interpolate_grads(F32, attr, rast, s["tri"], g)


@pytest.mark.parametrize("name", G.INTERP_SCENES)
@pytest.mark.parametrize("C", G.CHANNELS)
def test_interpolate_gradients(name, C):
    s = G.scene(name)
    attr, g, r64, r32 = interpolate_case(name, C)
    d_attr, d_rast = run_interpolate(attr, G.scene_rast(name), s["tri"], g)
    G.check_bars(f"{name} C={C} interpolate dL_dattr", d_attr, r64["d_attr"], r32["d_attr"], G.fixed_point_term(r64["B"], r64["n"]))
    G.check_bars(f"{name} C={C} interpolate dL_drast", d_rast, r64["d_rast"], r32["d_rast"])
    assert not d_rast[..., 2:].any()


@pytest.mark.parametrize("name", G.RAST_SCENES)
def test_rasterize_gradient(name):
    s = G.scene(name)
    g, n_amb, n_cov = uv_upstream(name)
    assert n_cov > 0 and n_amb <= 0.01 * n_cov, (n_amb, n_cov)
    r64, r32 = (G.rasterize_grads(f, s["pos"], s["tri"], device_rast(name), g) for f in (F64, F32))
    d_pos = run_rasterize(name, g)
    G.check_bars(f"{name} rasterize dL_dpos ({n_amb} of {n_cov} pixels at a clamp bound)", d_pos, r64["d_pos"], r32["d_pos"], G.fixed_point_term(r64["B"], r64["n"]))
    assert not d_pos[:, 2].any()


@functools.lru_cache(maxsize=None)
def antialias_case(name, C, boost=1.0):
    s = G.scene(name)
    color, g = A.colors(name, C), G.upstream(name, (s["H"], s["W"], C), "aa")
    args = (color, G.scene_rast(name), s["pos"], s["tri"], A.scene_topology(name), g, boost)
    return color, g, G.antialias_grads(F64, *args), G.antialias_grads(F32, *args)


@pytest.mark.parametrize("name", G.AA_GRAD_SCENES)
@pytest.mark.parametrize("C", G.CHANNELS)
def test_antialias_gradients(name, C):
    color, g, r64, r32 = antialias_case(name, C)
    d_color, d_pos, _ = run_antialias(name, color, g)
    G.check_bars(f"{name} C={C} antialias dL_dcolor", d_color, r64["d_color"], r32["d_color"])
    G.check_bars(f"{name} C={C} antialias dL_dpos ({len(r64['pairs']['R'])} pairs)", d_pos, r64["d_pos"], r32["d_pos"], G.fixed_point_term(r64["B"], r64["n"]))
    assert not d_pos[:, 2].any()


def test_pos_gradient_boost_and_topology_built_in_the_call():
    name, C = "ball_96", 3
    color, g, r64, r32 = antialias_case(name, C, 2.5)
    d_color, d_pos, _ = run_antialias(name, color, g, boost=2.5, topology=False)
    G.check_bars("ball_96 antialias dL_dpos, boost 2.5", d_pos, r64["d_pos"], r32["d_pos"], G.fixed_point_term(r64["B"], r64["n"]))
    plain_color, plain_pos, _ = run_antialias(name, color, g)
    assert np.array_equal(d_color, plain_color)                               # the boost is the pos gradient's alone
    assert np.abs(d_pos - 2.5 * plain_pos.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(d_pos).max()


# ---- one-hot upstreams -----------------------------------------------------------------------------------------------------------------
def _only_rows(grad, rows):
    return set(np.nonzero(grad.any(axis=-1))[0].tolist()) <= set(int(r) for r in rows)


@pytest.mark.parametrize("where", ["first", "last", "id_above_2^16"])
def test_one_hot_upstream_reaches_one_triangle(where):
    name, C = "tiny_256", 3
    s = G.scene(name)
    H, W, tri = s["H"], s["W"], np.asarray(s["tri"], np.int64)
    rast = device_rast(name)
    amb, _ = G.uv_ambiguous(s["pos"], s["tri"], rast)
    ids = rast[..., 3].astype(np.int64).reshape(-1)
    usable = (ids > 0) & ~amb.reshape(-1)
    pix = {"first": 0, "last": H * W - 1, "id_above_2^16": int(np.nonzero(usable & (ids > (1 << 16)))[0][0])}[where]
    assert usable[pix], "the pixel is covered and not at a clamp bound"
    verts = tri[ids[pix] - 1]
    # rasterize
    g4 = np.zeros((H, W, 4), np.float32)
    g4.reshape(-1, 4)[pix] = (0.75, -1.25, 3.0, 7.0)
    r64, r32 = (G.rasterize_grads(f, s["pos"], s["tri"], rast, g4) for f in (F64, F32))
    d_pos = run_rasterize(name, g4)
    assert _only_rows(d_pos, verts) and d_pos[verts].any()
    G.check_bars(f"tiny_256 one-hot {where} rasterize dL_dpos", d_pos, r64["d_pos"], r32["d_pos"], G.fixed_point_term(r64["B"], r64["n"]))
    # interpolate, on the same image
    attr = attrs(name, C)
    g = np.zeros((H, W, C), np.float32)
    g.reshape(-1, C)[pix] = (1.5, -0.5, 0.25)
    i64, i32 = (G.interpolate_grads(f, attr, rast, s["tri"], g) for f in (F64, F32))
    d_attr, d_rast = run_interpolate(attr, rast, s["tri"], g)
    assert _only_rows(d_attr, verts) and _only_rows(d_rast.reshape(-1, 4), [pix])
    G.check_bars(f"tiny_256 one-hot {where} interpolate dL_dattr", d_attr, i64["d_attr"], i32["d_attr"], G.fixed_point_term(i64["B"], i64["n"]))
    G.check_bars(f"tiny_256 one-hot {where} interpolate dL_drast", d_rast, i64["d_rast"], i32["d_rast"])


def test_one_hot_upstream_on_a_silhouette_pixel():
    name, C = "ball_96", 3
    s = G.scene(name)
    H, W = s["H"], s["W"]
    color = A.colors(name, C)
    pr = G.aa_pairs(G.scene_rast(name), s["pos"], s["tri"], A.scene_topology(name))
    R = int(pr["R"][len(pr["R"]) // 2])
    mine = pr["R"] == R
    g = np.zeros((H, W, C), np.float32)
    g.reshape(-1, C)[R] = (1.0, -2.0, 0.5)
    args = (color, G.scene_rast(name), s["pos"], s["tri"], A.scene_topology(name), g)
    r64, r32 = G.antialias_grads(F64, *args), G.antialias_grads(F32, *args)
    d_color, d_pos, _ = run_antialias(name, color, g)
    assert _only_rows(d_pos, np.concatenate([pr["va"][mine], pr["vb"][mine]])) and d_pos.any()
    assert _only_rows(d_color.reshape(-1, C), np.concatenate([[R], pr["O"][mine]]))
    G.check_bars("ball_96 one-hot silhouette antialias dL_dpos", d_pos, r64["d_pos"], r32["d_pos"], G.fixed_point_term(r64["B"], r64["n"]))
    G.check_bars("ball_96 one-hot silhouette antialias dL_dcolor", d_color, r64["d_color"], r32["d_color"])


def test_fullscreen_constant_upstream_goes_onto_four_vertices():
    """262 144 pixels with one sign onto four rows: the run reduction (every wave is one run) and the accumulator's headroom"""
    name = "fullscreen_512"
    s = G.scene(name)
    H, W = s["H"], s["W"]
    attr, rast = attrs(name, 1), G.scene_rast(name)
    g = np.full((H, W, 1), 1.75, np.float32)
    r64, r32 = (G.interpolate_grads(f, attr, rast, s["tri"], g) for f in (F64, F32))
    assert r64["n"] == H * W                                                  # vertices 0 and 2 are in both triangles
    d_attr, _ = run_interpolate(attr, rast, s["tri"], g)
    G.check_bars("fullscreen_512 constant upstream dL_dattr", d_attr, r64["d_attr"], r32["d_attr"], G.fixed_point_term(r64["B"], r64["n"]))
    assert abs(float(d_attr.sum()) - 1.75 * H * W) <= 2.0 ** -22 * 1.75 * H * W      # the three weights of a pixel add up to 1
    g4 = np.zeros((H, W, 4), np.float32)
    g4[..., 0], g4[..., 1] = 1.0, 0.5
    amb, _ = G.uv_ambiguous(s["pos"], s["tri"], device_rast(name))
    g4[amb] = 0.0
    p64, p32 = (G.rasterize_grads(f, s["pos"], s["tri"], device_rast(name), g4) for f in (F64, F32))
    G.check_bars("fullscreen_512 constant upstream dL_dpos", run_rasterize(name, g4), p64["d_pos"], p32["d_pos"], G.fixed_point_term(p64["B"], p64["n"]))


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_256", "tinypatch_128", "fullscreen_512"])
def test_two_runs_give_the_same_bits(name):
    s, C = G.scene(name), 3
    attr, g = attrs(name, C), G.upstream(name, (s["H"], s["W"], C), "twice")
    g4, color = G.upstream(name, (s["H"], s["W"], 4), "twice4"), A.colors(name, C)

    def once():
        return run_interpolate(attr, G.scene_rast(name), s["tri"], g) + (run_rasterize(name, g4),) + run_antialias(name, color, g)[:2]
    for a, b in zip(once(), once()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_batch_equals_its_images_summed_in_ascending_order():
    name, C, N = "flaps_64x48", 3, 3
    s, dr = G.scene(name), _dr()
    H, W, tri = s["H"], s["W"], _dev(s["tri"])
    scale = np.array([1.0, 0.9, 1.1], np.float32)[:, None, None] * np.array([1, 1, 1, 1], np.float32)
    scale[..., 3] = 1.0
    pos_b = np.asarray(s["pos"])[None] * scale                                # three different images of the mesh
    attr, g, g4 = attrs(name, C), G.upstream(name, (N, H, W, C), "batch")[..., :C], G.upstream(name, (N, H, W, 4), "batch4")
    colors = np.stack([A.colors(name, C), A.colors(name, C)[::-1].copy(), A.colors(name, C)[:, ::-1].copy()])
    # per-image pos [N,V,4]: rasterize and antialias; shared attr [V,C]: interpolate
    p, a, c = _dev(pos_b, True), _dev(attr, True), _dev(colors, True)
    rast, _ = dr.rasterize(None, p, tri, (H, W))
    rast.backward(_dev(g4))
    rast_d = rast.detach()
    out, _ = dr.interpolate(a, rast_d, tri)
    out.backward(_dev(g))
    d_pos_rast = p.grad.clone()
    p.grad = None
    dr.antialias(c, rast_d, p, tri).backward(_dev(g))
    shared = _dev(pos_b[0], True)                                             # shared pos [V,4] under three images of it
    rast0 = rast_d[0:1].expand(N, H, W, 4).contiguous()
    dr.antialias(c.detach(), rast0, shared, tri).backward(_dev(g))
    total_attr, total_shared = None, None
    for n in range(N):
        pn, an, cn, sn = _dev(pos_b[n], True), _dev(attr, True), _dev(colors[n:n + 1], True), _dev(pos_b[0], True)
        r1, _ = dr.rasterize(None, pn, tri, (H, W))
        assert torch.equal(r1[0], rast_d[n])
        r1.backward(_dev(g4[n:n + 1]))
        assert torch.equal(pn.grad, d_pos_rast[n])
        pn.grad = None
        dr.interpolate(an, rast_d[n:n + 1], tri)[0].backward(_dev(g[n:n + 1]))
        total_attr = an.grad if total_attr is None else total_attr + an.grad
        dr.antialias(cn, rast_d[n:n + 1], pn, tri).backward(_dev(g[n:n + 1]))
        assert torch.equal(pn.grad, p.grad[n]) and torch.equal(cn.grad[0], c.grad[n])
        dr.antialias(cn.detach(), rast_d[0:1], sn, tri).backward(_dev(g[n:n + 1]))
        total_shared = sn.grad if total_shared is None else total_shared + sn.grad
    assert torch.equal(a.grad, total_attr) and torch.equal(shared.grad, total_shared)
    assert a.grad.any() and shared.grad.any() and p.grad.any()


def test_no_faces_or_no_vertices_gives_zeros_and_the_upstream():
    dr = _dr()
    H, W, C = 9, 7, 2
    g, g4 = _dev(G.upstream("empty", (1, H, W, C), "e")), _dev(G.upstream("empty", (1, H, W, 4), "e4"))
    for V, F in ((5, 0), (0, 2), (0, 0)):
        pos = _dev(np.random.default_rng(1).uniform(0.5, 1.0, (V, 4)).astype(np.float32), True)
        tri = _dev(np.tile(np.array([[0, 1, 2]], np.int32), (F, 1)).reshape(F, 3))
        attr, color = _dev(np.ones((V, C), np.float32), True), _dev(G.upstream("empty", (1, H, W, C), "c"), True)
        rast, _ = dr.rasterize(None, pos, tri, (H, W), validate=False)
        assert not rast.any()
        rast.backward(g4)
        assert pos.grad.shape == (V, 4) and not pos.grad.any()
        pos.grad = None
        r = rast.detach().clone().requires_grad_(True)
        dr.interpolate(attr, r, tri)[0].backward(g)
        assert attr.grad.shape == (V, C) and not attr.grad.any() and not r.grad.any()
        dr.antialias(color, rast.detach(), pos, tri).backward(g)
        assert torch.equal(color.grad, g) and not pos.grad.any()


def test_a_nan_upstream_is_loud_in_its_gradient_and_nowhere_else():
    name, C = "ball_96", 3
    s = G.scene(name)
    H, W = s["H"], s["W"]
    pr = G.aa_pairs(G.scene_rast(name), s["pos"], s["tri"], A.scene_topology(name))
    R = int(pr["R"][0])                                                       # a covered pixel or its neighbour, a receiver of a blend
    near = [R + d for d in (0, -1, 1, -W, W)]
    g = G.upstream(name, (H, W, C), "nan")
    clean = run_antialias(name, A.colors(name, C), g)
    g[R // W, R % W, 1] = np.nan
    d_color, d_pos, _ = run_antialias(name, A.colors(name, C), g)
    assert np.isnan(d_pos).all()                                              # the scatter: every element, the z column too
    rest = np.ones(H * W, bool)
    rest[near] = False
    assert np.isnan(d_color.reshape(-1, C)[R]).any() and np.array_equal(d_color.reshape(-1, C)[rest], clean[0].reshape(-1, C)[rest])
    # interpolate: dL_dattr is the scatter, dL_drast is per pixel
    cov = int(np.nonzero(G.scene_rast(name)[..., 3].reshape(-1) > 0)[0][5])
    gi = G.upstream(name, (H, W, C), "nan_i")
    clean_attr, clean_rast = run_interpolate(attrs(name, C), G.scene_rast(name), s["tri"], gi)
    gi.reshape(-1, C)[cov, 0] = np.nan
    d_attr, d_rast = run_interpolate(attrs(name, C), G.scene_rast(name), s["tri"], gi)
    others = np.arange(H * W) != cov
    assert np.isnan(d_attr).all() and np.isfinite(clean_attr).all()
    assert np.isnan(d_rast.reshape(-1, 4)[cov, :2]).all() and np.array_equal(d_rast.reshape(-1, 4)[others], clean_rast.reshape(-1, 4)[others])
    # rasterize: a NaN on the z/w or the ID channel is ignored; on u it is loud
    g4 = G.upstream(name, (H, W, 4), "nan_r")
    want = run_rasterize(name, g4)
    g4.reshape(-1, 4)[cov, 2:] = np.nan
    assert np.array_equal(run_rasterize(name, g4), want) and np.isfinite(want).all()
    g4.reshape(-1, 4)[cov, 0] = np.nan
    assert np.isnan(run_rasterize(name, g4)).all()


def test_nothing_is_launched_for_an_input_without_a_gradient():
    """only the wanted gradients exist, and they are the bits of the call that wanted all of them"""
    name, C = "flaps_64x48", 3
    s, dr = G.scene(name), _dr()
    attr, g, color = attrs(name, C), G.upstream(name, (s["H"], s["W"], C), "part"), A.colors(name, C)
    both_attr, both_rast = run_interpolate(attr, G.scene_rast(name), s["tri"], g)
    both_color, both_pos, _ = run_antialias(name, color, g)
    tri, rast = _dev(s["tri"]), _dev(G.scene_rast(name))[None]
    for want_attr in (True, False):
        a, r = _dev(attr, want_attr), rast.clone().requires_grad_(not want_attr)
        dr.interpolate(a, r, tri)[0].backward(_dev(g)[None])
        assert (a.grad is None) == (not want_attr) and (r.grad is None) == want_attr
        assert np.array_equal(_np(a.grad), both_attr) if want_attr else np.array_equal(_np(r.grad[0]), both_rast)
    for want_color in (True, False):
        c, p = _dev(color, want_color), _dev(s["pos"], not want_color)
        dr.antialias(c[None], rast, p, tri).backward(_dev(g)[None])
        assert (c.grad is None) == (not want_color) and (p.grad is None) == want_color
        assert np.array_equal(_np(c.grad), both_color) if want_color else np.array_equal(_np(p.grad), both_pos)


@pytest.mark.parametrize("folded,n_pairs,n_covered", [(False, 28, (48, 24)), (True, 32, (27, 3))])
def test_the_two_id_rules_stay_two(folded, n_pairs, n_covered):
    """An ID of F + 0.5: antialias truncates it and still sees triangle F (aa_id), interpolate sees nothing (mesh_pixel_triangle); forward and
    backward of both.  The counts are the restatements' own, so that nothing here passes vacuously."""
    dr, C = _dr(), 3
    pos, tri, rast = A.quad_case(folded)
    H, W, F, V = rast.shape[0], rast.shape[1], len(tri), len(pos)
    hit = rast[..., 3] == F
    half = rast.copy()
    half[hit, 3] = F + 0.5
    rng = np.random.default_rng(11 + folded)
    color, attr, g = (rng.uniform(-1.0, 1.0, s).astype(np.float32) for s in ((H, W, C), (V, C), (H, W, C)))
    topo = A.topology(tri, V)
    assert int(hit.sum()) == 24 and len(G.aa_pairs(rast, pos, tri, topo)["R"]) == len(G.aa_pairs(half, pos, tri, topo)["R"]) == n_pairs
    assert (len(G.covered(rast, tri, V)[0]), len(G.covered(half, tri, V)[0])) == n_covered

    def both(r):
        c, p, a, rd = _dev(color, True), _dev(pos, True), _dev(attr, True), _dev(r, True)
        out = dr.antialias(c[None], _dev(r)[None], p, _dev(tri))
        out.backward(_dev(g)[None])
        val, _ = dr.interpolate(a, rd[None], _dev(tri))
        val.backward(_dev(g)[None])
        return [_np(t) for t in (out[0], c.grad, p.grad, val[0], a.grad, rd.grad)]
    (aa0, dc0, dp0, val0, _, _), (aa1, dc1, dp1, val1, d_attr, d_rast) = both(rast), both(half)
    for got, want in ((aa1, aa0), (dc1, dc0), (dp1, dp0)):                    # antialias: the bits of the unmodified rast
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(dp0).max() > 0 and not np.array_equal(aa0, color)
    assert not val1[hit].any() and np.array_equal(val1[~hit].view(np.uint32), val0[~hit].view(np.uint32)) and val0[hit].any()
    assert not d_rast[hit].any()
    r64, r32 = (G.interpolate_grads(f, attr, half, tri, g) for f in (F64, F32))
    G.check_bars(f"quad folded={folded} ID F + 0.5 interpolate dL_dattr", d_attr, r64["d_attr"], r32["d_attr"], G.fixed_point_term(r64["B"], r64["n"]))


def test_a_parameter_goes_where_a_tensor_goes():
    """pos [V,4] and attr [V,C] as torch.nn.Parameter, the usual leaf of a mesh fit: trainable through the three calls, frozen through the
    forward-only modules.  Outputs and gradients have the bits of the plain-tensor calls."""
    import youreditableavatar_amd.mesh_raster_aa as fwd
    name, C = "flaps_64x48", 3
    s, dr = G.scene(name), _dr()
    H, W, tri = s["H"], s["W"], _dev(s["tri"])
    g4, g = _dev(G.upstream(name, (1, H, W, 4), "par4")), _dev(G.upstream(name, (1, H, W, C), "par"))
    color = _dev(A.colors(name, C))[None]
    bits = lambda t: t.detach().view(torch.int32)

    def run(leaf):
        p, a = leaf(_dev(s["pos"])), leaf(_dev(attrs(name, C)))
        rast, _ = dr.rasterize(None, p, tri, (H, W))
        rast.backward(g4)
        d_pos_rast, p.grad = p.grad, None
        out, _ = dr.interpolate(a, rast.detach(), tri)
        out.backward(g)
        aa = dr.antialias(color, rast.detach(), p, tri)
        aa.backward(g)
        return rast, d_pos_rast, out, a.grad, aa, p.grad
    plain, param = run(lambda t: t.requires_grad_(True)), run(torch.nn.Parameter)
    for x, y in zip(plain, param):
        assert torch.equal(bits(x), bits(y))
    assert plain[1].any() and plain[3].any() and plain[5].any()
    pos_f, attr_f = (torch.nn.Parameter(_dev(a), requires_grad=False) for a in (s["pos"], attrs(name, C)))
    rast, _ = fwd.rasterize(None, pos_f, tri, (H, W))
    assert torch.equal(bits(rast), bits(plain[0])) and torch.equal(bits(fwd.interpolate(attr_f, rast, tri)[0]), bits(plain[2]))
    assert torch.equal(bits(fwd.antialias(color, rast, pos_f, tri)), bits(plain[4]))


# ---- the chain and the example ---------------------------------------------------------------------------------------------------------
def _chain(pos, vn, uv, vid, pix, pr, HW, g_n, g_o):
    """rasterize -> interpolate -> normalize / lerp -> antialias -> loss, in torch, on given decisions (pos, vn: leaves of any dtype)"""
    H, W = HW
    f = pos.dtype
    nrm = torch.zeros((H * W, 3), dtype=f).index_add(0, torch.from_numpy(pix), G.interpolate_torch(vn[torch.from_numpy(vid).reshape(-1)].reshape(-1, 3, 3), uv))
    mask = torch.zeros((H * W, 1), dtype=f)
    mask[pix] = 1.0
    img = torch.lerp(torch.zeros_like(nrm), (torch.nn.functional.normalize(nrm, dim=-1) + 1.0) / 2.0, mask)
    PA, PB = pos[torch.from_numpy(pr["va"])], pos[torch.from_numpy(pr["vb"])]
    return (G.aa_torch(img, PA, PB, pr, W, H) * g_n).sum() + (G.aa_torch(mask, PA, PB, pr, W, H) * g_o).sum()


def test_the_whole_chain_against_the_reference():
    name = "ball_96"
    s, dr = G.scene(name), _dr()
    H, W = s["H"], s["W"]
    rng = np.random.default_rng(77)
    vn = rng.normal(size=(len(s["pos"]), 3)).astype(np.float32)
    g_n, g_o = G.upstream(name, (H, W, 3), "chain_n"), G.upstream(name, (H, W, 1), "chain_o")
    amb, n_cov = G.uv_ambiguous(s["pos"], s["tri"], device_rast(name))
    assert not amb.any()                                                      # (ball_96: no covered pixel at a clamp bound)
    pos_d, vn_d, tri = _dev(s["pos"], True), _dev(vn, True), _dev(s["tri"])
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos_d, tri, (H, W))
    nrm, _ = dr.interpolate(vn_d, rast, tri)
    mask = (rast[..., 3:] > 0).float()
    img = torch.lerp(torch.zeros_like(nrm), (torch.nn.functional.normalize(nrm, dim=-1) + 1.0) / 2.0, mask)
    loss = (dr.antialias(img, rast, pos_d, tri) * _dev(g_n)[None]).sum() + (dr.antialias(mask, rast, pos_d, tri) * _dev(g_o)[None]).sum()
    loss.backward()
    host_rast = device_rast(name)
    pix, vid = G.covered(host_rast, s["tri"], len(s["pos"]))
    pr = G.aa_pairs(host_rast, s["pos"], s["tri"], A.scene_topology(name))
    assert len(pr["R"]) > 100
    ref = {}
    for f in (F64, F32):
        p, v = G._t(s["pos"], f).requires_grad_(True), G._t(vn, f).requires_grad_(True)
        u_, v_, _, _ = G.uv_torch(p[torch.from_numpy(vid).reshape(-1)].reshape(-1, 3, 4), torch.from_numpy(pix % W), torch.from_numpy(pix // W), W, H)
        _chain(p, v, torch.stack([u_, v_], 1), vid, pix, pr, (H, W), G._t(g_n.reshape(-1, 3), f), G._t(g_o.reshape(-1, 1), f)).backward()
        ref[f] = (p.grad.double().numpy(), v.grad.double().numpy())
    G.check_bars("ball_96 chain dL_dpos", _np(pos_d.grad), ref[F64][0], ref[F32][0])
    G.check_bars("ball_96 chain dL_dvn", _np(vn_d.grad), ref[F64][1], ref[F32][1])


def test_the_example_lowers_its_loss_through_the_silhouette_gradient():
    spec = importlib.util.spec_from_file_location("fit_mesh_silhouette_normals", os.path.join(ROOT, "examples", "fit_mesh_silhouette_normals.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.fit(resolution=96, steps=40, verbose=False)
    print(f"fit_mesh_silhouette_normals at 96^2, 40 steps: loss {res['first_loss']:.5f} -> {res['last_loss']:.5f} (factor {res['first_loss'] / res['last_loss']:.2f})")
    assert res["last_loss"] < res["first_loss"]
    assert res["silhouette_vertices"] > 0 and res["silhouette_grad_nonzero"] > 0
