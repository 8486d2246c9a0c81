"""CPU: the restatement of the tetrahedral grid's passes (tests/tet_ref.py) against what the reference's own compact_tets, batch_subdivide_volume and
mark_part_tets returned (tests/golden/ref_tet_grid_fixture.npz), element for element -- floats compared as bits, NaN positions included -- and
the properties of a subdivision on kuhn_16."""
import numpy as np
import pytest
import torch

from tests import tet_ref as T


def _compare(prefix, keys, got):
    fx = T.fixture()
    for k, g in zip(keys, got):
        if g is None:
            assert f"{prefix}.{k}" not in fx, (prefix, k)
        else:
            T.assert_same(g, fx[f"{prefix}.{k}"], f"{prefix}.{k}")


@pytest.mark.parametrize("name", T.FIXTURE_SCENES)
@pytest.mark.parametrize("with_mask", [False, True])
def test_the_restatement_equals_the_fixture(name, with_mask):
    fx = T.fixture()
    s = T.scene(name)
    for k in ("pos", "sdf", "tet", "mask"):
        T.assert_same(s[k], fx[f"{name}.{k}"], k)                              # the scene is the one that was recorded
    pos, sdf, tet, mask = T.tensors(name)
    m, tag = (mask, "_mask") if with_mask else (None, "")
    c = T.compact_tets(pos, sdf, tet, m)
    _compare(f"{name}.compact{tag}", T.COMPACT_KEYS, c)
    batched = lambda o: (o[0][None], o[1][None], None if o[2] is None else o[2][None], o[3])
    _compare(f"{name}.subdiv{tag}", T.SUBDIV_KEYS, batched(T.subdivide_tets(pos, tet, m)))
    _compare(f"{name}.chain{tag}", T.SUBDIV_KEYS, batched(T.subdivide_tets(c[0], c[2], c[3])))


@pytest.mark.parametrize("name", T.FIXTURE_SCENES)
def test_mark_part_tets_equals_the_fixture(name):
    pos, sdf, tet, _ = T.tensors(name)
    out = T.mark_part_tets(pos, sdf, tet, torch.from_numpy(T.fixture()[f"{name}.edit_mask"]))
    _compare(f"{name}.mark", T.MARK_KEYS, [out[k] for k in T.MARK_KEYS])


def test_odd_holds_what_it_is_there_for():
    s = T.odd()
    tet, sdf, mask = s["tet"].copy(), s["sdf"].copy(), s["mask"][:, 0]
    assert (tet[:, :-1] > tet[:, 1:]).any() and (tet[:, :-1] < tet[:, 1:]).any()
    assert len(np.unique(tet, axis=0)) < len(tet) and any(len(set(r)) < 4 for r in tet.tolist())
    assert len(np.setdiff1d(np.arange(len(sdf)), tet)) >= 3 and np.isnan(sdf[tet]).any() and np.isinf(sdf[tet]).any()
    kept = T.selection(torch.from_numpy(sdf), torch.from_numpy(tet)).numpy()
    rows = sdf[tet]
    assert kept[(rows == T.T02).all(1)].all() and (rows == T.T02).all(1).sum() >= 2
    assert not kept[(rows == T.ABOVE).all(1)].any() and (rows == T.ABOVE).all(1).sum() >= 2 and T.ABOVE > T.T02
    assert kept[(rows == -T.T02).all(1)].all() and (rows == -T.T02).all(1).sum() >= 2
    assert not kept[~np.isfinite(rows).all(1)].any()
    edges = T.subdivide_tets(torch.from_numpy(s["pos"].copy()), torch.from_numpy(tet))[4].numpy()
    assert set((mask[edges[:, 0]] + mask[edges[:, 1]]).tolist()) == {0, 1, 2}
    assert (edges[:, 0] == edges[:, 1]).any()                                  # the edge (v, v) of the repeated vertex is an edge like any other


def test_the_properties_of_a_subdivision():
    pos, _, tet, _ = T.tensors("kuhn_16")
    new_v, new_tets, _, parents, edges = T.whole("kuhn_16")
    N, E, F = len(pos), len(edges), len(tet)
    e = edges.numpy()
    key = e[:, 0] * (N + 1) + e[:, 1]
    assert (e[:, 0] <= e[:, 1]).all() and (key[1:] > key[:-1]).all()           # strictly ascending
    assert new_v.shape == (N + E, 3) and new_tets.shape == (8 * F, 4) and int(new_tets.max()) < N + E and int(new_tets.min()) >= 0
    assert np.array_equal(np.unique(new_tets.numpy()[new_tets.numpy() >= N]), np.arange(N, N + E))   # every index at or above N is used
    assert np.array_equal(parents.numpy(), np.tile(np.arange(F), 8))
    # the eight children fill their parent: their volumes add up to its volume
    vol = lambda v, t: np.abs(np.linalg.det((v[t[:, 1:]] - v[t[:, :1]]).astype(np.float64))) / 6.0
    parent_vol = vol(pos.numpy(), tet.numpy())
    child_vol = vol(new_v.numpy(), new_tets.numpy()).reshape(8, F)
    assert (child_vol > 0).all() and np.allclose(child_vol.sum(0), parent_vol, rtol=1e-4)
