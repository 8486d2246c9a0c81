"""GPU: youreditableavatar_amd.tet_grid against what the reference's own compact_tets, batch_subdivide_volume and mark_part_tets returned
(tests/golden/ref_tet_grid_fixture.npz: odd, kuhn_8) and against the restatement (tests/tet_ref.py: kuhn_16, kuhn_32).

Everything is integer topology, bit copies and exact halvings: every integer must be equal and every float bit-equal (NaN positions included).
There are no tolerances, except on the vertices of the marching tetrahedra at the end of the chain, which keep their own rule (4 eta)."""
import numpy as np
import pytest
import torch

from tests import mt_ref as R
from tests import tet_ref as T

pytestmark = pytest.mark.gpu
I64, I32 = torch.int64, torch.int32


def _tg():
    import youreditableavatar_amd.tet_grid as tg
    return tg


def _same(prefix, keys, got, want):
    assert len(got) == len(keys) == len(want)
    for k, g, w in zip(keys, got, want):
        if w is None:
            assert g is None, (prefix, k)
        else:
            assert g.is_cuda and not g.requires_grad, (prefix, k)
            T.assert_same(g, w, f"{prefix}.{k}")


def _fx(prefix, keys):
    fx = T.fixture()
    return [fx.get(f"{prefix}.{k}") for k in keys]


def _unbatched(want):
    return [None if w is None else w[0] for w in want[:3]] + [want[3]]


# ---- against the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.FIXTURE_SCENES)
@pytest.mark.parametrize("idx", [I64, I32])
@pytest.mark.parametrize("column", [False, True])
def test_compact_and_subdivide_equal_the_fixture(name, idx, column):
    tg = _tg()
    pos, sdf, tet, mask = T.tensors(name, "cuda", column)
    tet = tet.to(idx)
    for tag, m in (("", None), ("_mask", mask)):
        want = _fx(f"{name}.compact{tag}", T.COMPACT_KEYS)
        if not column:
            want[1] = want[1].reshape(-1)
        for out_dtype in (I64, I32):
            c = tg.compact_tets(pos, sdf, tet, m, index_dtype=out_dtype)
            assert c[2].dtype == c[4].dtype == out_dtype and c[0].dtype == c[1].dtype == torch.float32 and (m is None or c[3].dtype == m.dtype)
            _same(f"{name}.compact{tag}", T.COMPACT_KEYS, c, want)
            d = tg.subdivide_tets(c[0], c[2], c[3])                              # the compacted grid, int32 or int64 rows as they come
            assert d[1].dtype == d[3].dtype == d[4].dtype == I64 and (m is None or d[2].dtype == torch.float32)
            _same(f"{name}.chain{tag}", T.SUBDIV_KEYS, d[:4], _unbatched(_fx(f"{name}.chain{tag}", T.SUBDIV_KEYS)))
        w = tg.subdivide_tets(pos, tet, m if column or m is None else m[:, 0])
        _same(f"{name}.subdiv{tag}", T.SUBDIV_KEYS, w[:4], _unbatched(_fx(f"{name}.subdiv{tag}", T.SUBDIV_KEYS)))
        assert w[4].shape == (len(w[0]) - len(pos), 2)
        b = tg.batch_subdivide_volume(pos[None], tet[None], None if m is None else m[None])
        _same(f"{name}.subdiv{tag} (batched)", T.SUBDIV_KEYS, b, _fx(f"{name}.subdiv{tag}", T.SUBDIV_KEYS))


@pytest.mark.parametrize("name", T.FIXTURE_SCENES)
@pytest.mark.parametrize("idx", [I64, I32])
def test_mark_part_tets_equals_the_fixture(name, idx):
    pos, sdf, tet, _ = T.tensors(name, "cuda")
    edit = torch.from_numpy(T.fixture()[f"{name}.edit_mask"]).cuda()
    out = _tg().mark_part_tets(pos, sdf, tet.to(idx), edit)
    assert tuple(out) == T.MARK_KEYS and out["mask_keep_part_in_new_pos"].dtype == I32
    _same(f"{name}.mark", T.MARK_KEYS, [out[k] for k in T.MARK_KEYS], _fx(f"{name}.mark", T.MARK_KEYS))


# ---- against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kuhn_16", "kuhn_32"])
@pytest.mark.parametrize("threshold", [0.02, 0.1])
def test_compact_then_subdivide_equals_the_restatement(name, threshold):
    tg = _tg()
    want_c, want_d = T.chain(name, threshold)
    pos, sdf, tet, mask = T.tensors(name, "cuda")
    c = tg.compact_tets(pos, sdf, tet, mask, threshold=threshold)
    _same(f"{name} compact at {threshold}", T.COMPACT_KEYS, c, want_c)
    assert 0 < len(c[4]) < len(tet)
    d = tg.subdivide_tets(c[0], c[2], c[3])
    _same(f"{name} subdivided", T.SUBDIV_KEYS + ("edges",), d, want_d)
    if (name, threshold) == ("kuhn_32", 0.02):                                   # constants taken from the reference's methods on the CPU
        assert (len(c[4]), len(c[0]), len(d[4]), len(d[1])) == (13524, 4885, 23646, 108192)


@pytest.mark.parametrize("name", ["kuhn_16", "kuhn_32"])
def test_the_whole_grid_subdivided_equals_the_restatement(name):
    """24 576 and 196 608 rows, every interior edge shared by four to six of them; at kuhn_32 the scans over N + 1 take their second level"""
    pos, _, tet, mask = T.tensors(name, "cuda")
    _same(f"{name} whole", T.SUBDIV_KEYS + ("edges",), _tg().subdivide_tets(pos, tet.int() if name == "kuhn_16" else tet, mask), T.whole(name))


def test_subdividing_twice():
    """num_subdiv = 2: the output is a valid input, the float mask included"""
    tg = _tg()
    pos, _, tet, mask = T.tensors("kuhn_8", "cuda")
    once = tg.subdivide_tets(pos, tet, mask)
    twice = tg.subdivide_tets(once[0], once[1], once[2])
    p, _, t, m = T.tensors("kuhn_8")
    ref = T.subdivide_tets(*T.subdivide_tets(p, t, m)[:3])
    _same("kuhn_8 twice", T.SUBDIV_KEYS + ("edges",), twice, ref)
    assert len(twice[1]) == 64 * len(tet)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def _sphere(new_v):
    """sdf = 0.37 - |x - 1/2| on the new vertices: evaluated once, in double on the host from the (bit-equal) positions, then rounded"""
    v = new_v.detach().cpu().numpy().astype(np.float64)
    return torch.from_numpy((0.37 - np.linalg.norm(v - 0.5, axis=1)).astype(np.float32))


@pytest.mark.parametrize("name,threshold,n_verts,n_faces", [("kuhn_16", 0.1, 7970, 15936), ("kuhn_8", 0.15, 2013, 4022)])
def test_the_chain_into_marching_tets(name, threshold, n_verts, n_faces):
    import youreditableavatar_amd.marching_tets as mt
    tg = _tg()
    pos, sdf, tet, _ = T.tensors(name, "cuda")
    c = tg.compact_tets(pos, sdf, tet, threshold=threshold)
    new_v, new_tets, _, parents, _ = tg.subdivide_tets(c[0], c[2])
    fine = _sphere(new_v)
    out = mt.marching_tets(new_v, fine.cuda(), new_tets)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (len(got["verts"]), len(got["faces"])) == (n_verts, n_faces)
    m = R.manifold_counts(got["faces"], len(got["verts"]))                        # one wrongly merged or duplicated edge breaks these
    assert m == dict(directed_repeated=0, undirected_not_two=0, euler=2, unused_verts=0), m
    # the restatement's chain on the CPU
    p, s, t, _ = T.tensors(name)
    rc = T.compact_tets(p, s, t, threshold=threshold)
    rv, rt, _, rp, _ = T.subdivide_tets(rc[0], rc[2])
    T.assert_same(new_v, rv, "new_v"); T.assert_same(new_tets, rt, "new_tets")
    ref64, ref32 = (R.marching_tets(rv.to(f), fine.to(f), rt) for f in (torch.float64, torch.float32))
    for k in ("faces", "face_to_tet_idx", "valid_tets", "interp_v"):
        assert np.array_equal(got[k], ref64[k].numpy()), k
    v64 = ref64["verts"].numpy()
    eta, err = float(np.abs(ref32["verts"].double().numpy() - v64).max()), float(np.abs(got["verts"] - v64).max())
    print(f"{name} chain verts: eta {eta:.3g} err {err:.3g}")
    assert err <= 4.0 * eta, (err, eta)
    # every face's coarse tetrahedron is one the coarse marching tetrahedra call valid, or one the selection kept
    coarse_valid = mt.marching_tets(pos, sdf, tet)["valid_tets"]
    kept = torch.zeros(len(tet), dtype=torch.bool, device="cuda")
    kept[c[4]] = True
    origin = c[4][parents[out["face_to_tet_idx"]]]
    assert bool((coarse_valid | kept)[origin].all())
    assert bool(kept[coarse_valid].all())                                         # the selection keeps every crossing tetrahedron of the coarse grid
    if name == "kuhn_16":
        assert int(coarse_valid.sum()) == 3132


def test_two_calls_give_the_same_bytes():
    tg = _tg()
    pos, sdf, tet, mask = T.tensors("kuhn_32", "cuda")
    edit = None
    runs = []
    for _ in range(2):
        c = tg.compact_tets(pos, sdf, tet, mask, threshold=0.1)
        d = tg.subdivide_tets(c[0], c[2], c[3])
        p, s, t, _ = T.tensors("kuhn_8", "cuda")
        if edit is None:
            import youreditableavatar_amd.marching_tets as mt
            edit = (torch.arange(len(mt.marching_tets(p, s, t)["faces"]), device="cuda") % 3 == 0).int()
        k = _tg().mark_part_tets(p, s, t, edit)
        runs.append([x.cpu().numpy() for x in (*c, *d, *k.values())])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- the edges of the domain -----------------------------------------------------------------------------------------------------------
def test_nothing_kept_and_no_tetrahedra():
    tg = _tg()
    pos, sdf, tet, mask = T.tensors("kuhn_8", "cuda")
    for column, F, thr in ((True, len(tet), -1.0), (False, len(tet), 0.0), (True, 0, 0.02), (False, 0, 0.02)):
        s = sdf if column else sdf[:, 0] + 5.0
        c = tg.compact_tets(pos, s, tet[:F], mask, threshold=thr)
        assert [tuple(x.shape) for x in c] == [(0, 3), (0, 1) if column else (0,), (0, 4), (0, 1), (0,)]
        assert [x.dtype for x in c] == [torch.float32, torch.float32, I64, I32, I64]
    new_v, new_tets, new_mask, parents, edges = tg.subdivide_tets(pos, tet[:0], mask)
    assert new_v is pos and tuple(new_tets.shape) == (0, 4) and tuple(parents.shape) == (0,) and tuple(edges.shape) == (0, 2)
    T.assert_same(new_mask, mask.float().cpu(), "mask")
    b = tg.batch_subdivide_volume(pos[None], tet[None, :0])
    assert tuple(b[0].shape) == (1, len(pos), 3) and tuple(b[1].shape) == (1, 0, 4) and b[2] is None


def test_an_index_out_of_range_raises_and_the_device_stays_usable():
    """an argument check: the flag travels with the counts, the kernels never read through the index"""
    tg = _tg()
    pos, sdf, tet, _ = T.tensors("kuhn_8", "cuda")
    N = len(pos)
    for bad, idx in ((N, I64), (-1, I32), (1 << 40, I64)):
        t = tet.clone()
        t[len(t) // 2, 2] = bad
        t = t.to(idx) if idx == I64 else t.int()
        with pytest.raises(RuntimeError, match=r"outside \[0, 729\)"):
            tg.compact_tets(pos, sdf, t, threshold=10.0)
        with pytest.raises(RuntimeError, match=r"outside \[0, 729\)"):
            tg.subdivide_tets(pos, t)
        with pytest.raises(RuntimeError, match=r"outside \[0, 729\)"):
            tg.batch_subdivide_volume(pos[None], t[None])
    c = tg.compact_tets(pos, sdf, tet)
    _same("kuhn_8.compact", T.COMPACT_KEYS, c, _fx("kuhn_8.compact", T.COMPACT_KEYS))


def test_cpu_tensors_raise():
    tg = _tg()
    pos, sdf, tet, mask = T.tensors("kuhn_8", "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        tg.compact_tets(pos.cpu(), sdf.cpu(), tet.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        tg.subdivide_tets(pos, tet.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        tg.compact_tets(pos, sdf, tet, mask.cpu())


def test_positions_that_require_a_gradient():
    """d new_v.sum() / d pos[v] = 1 + 1/2 per distinct edge at v, in every coordinate; compact_tets detaches"""
    tg = _tg()
    pos, sdf, tet, mask = T.tensors("kuhn_8", "cuda")
    pos = pos.requires_grad_(True)
    assert not any(x.requires_grad for x in tg.compact_tets(pos, sdf.requires_grad_(True), tet, mask))
    new_v, new_tets, new_mask, parents, edges = tg.subdivide_tets(pos, tet, mask)
    assert new_v.requires_grad and not new_tets.requires_grad and not edges.requires_grad
    want = T.whole("kuhn_8")
    _same("kuhn_8 whole", T.SUBDIV_KEYS[1:] + ("edges",), [new_tets, new_mask, parents, edges], want[1:])
    T.assert_same(new_v.detach(), want[0], "new_v")                               # ((a + b) / 2 and (a + b) * 0.5f are the same float)
    new_v.sum().backward()
    at = np.bincount(want[4].numpy().reshape(-1), minlength=len(pos))
    assert np.array_equal(pos.grad.cpu().numpy(), np.repeat((1.0 + 0.5 * at)[:, None], 3, 1).astype(np.float32))
    with torch.no_grad():
        assert not tg.subdivide_tets(pos, tet)[0].requires_grad


def test_two_batch_elements_with_their_own_positions():
    tg = _tg()
    pos, _, tet, mask = T.tensors("kuhn_8", "cuda")
    pos2 = torch.stack([pos, pos.flip(0) * 1.5 - 0.25])
    mask2 = torch.stack([mask, 1 - mask])
    new_v, new_tets, new_mask, parents = tg.batch_subdivide_volume(pos2, torch.stack([tet, tet]), mask2)
    assert tuple(new_tets.shape) == (2, 8 * len(tet), 4) and new_v.shape[0] == new_mask.shape[0] == 2
    for b in range(2):
        want = T.subdivide_tets(pos2[b].cpu(), tet.cpu(), mask2[b].cpu())
        _same(f"batch element {b}", T.SUBDIV_KEYS, [new_v[b], new_tets[b], new_mask[b], parents], want[:4])
