"""CPU: the restatement of the hash-grid field's rules (tests/hashgrid_ref.py) against the figures of the reference's default config, against a slow
per-point loop, at x = 1.0, under the kink cap, and under float64 gradcheck; and youreditableavatar_amd.hashgrid.level_table against the same figures."""
import numpy as np
import pytest
import torch

from tests import hashgrid_ref as R

DEFAULT_RESOLUTIONS = [16, 23, 31, 43, 59, 81, 112, 154, 213, 295, 407, 562, 777, 1073, 1483, 2048]
DEFAULT_DENSE_SIZES = [4096, 12168, 29792, 79512, 205384]


def _tables(name):
    from youreditableavatar_amd import hashgrid
    ours = hashgrid.level_table(R.CONFIGS[name])
    ref = R.level_table(R.CONFIGS[name])
    assert [tuple(v) for v in ours] == [tuple(v) for v in ref], name
    return ours


def test_the_default_level_table_to_the_digit():
    lv = _tables("default")
    assert [v.resolution for v in lv] == DEFAULT_RESOLUTIONS
    assert [v.size for v in lv[:5]] == DEFAULT_DENSE_SIZES and all(v.dense for v in lv[:5])
    assert all(v.size == 1 << 19 and not v.dense for v in lv[5:])
    assert [v.offset for v in lv] == list(np.concatenate([[0], np.cumsum([v.size for v in lv])[:-1]]))
    assert sum(v.size for v in lv) == 6098120 and 2 * R.n_entries(lv) == 12196240
    assert lv[0].scale == 15.0 and abs(lv[15].scale - 2046.9987) < 1e-3 and np.float32(lv[15].scale) == lv[15].scale
    from youreditableavatar_amd import hashgrid
    assert hashgrid.HashGrid(3, R.CONFIGS["default"]).params.numel() == 12196240


def test_the_small_level_tables():
    tiny, odd = _tables("tiny"), _tables("odd")
    assert [(v.resolution, v.size, v.dense) for v in tiny] == [(2, 8, True), (4, 64, True), (8, 64, False), (16, 64, False)]   # 4^3 == 64: the boundary of dense
    assert [v.size for v in odd] == [32, 128, 256, 256, 256] and [v.resolution for v in odd[:2]] == [3, 5]                    # 27 -> 32 and 125 -> 128
    assert [v.dense for v in odd] == [True, True, False, False, False]


@pytest.mark.parametrize("set_name", R.POINT_SETS)
def test_the_restatement_against_a_slow_loop(set_name):
    levels, P = R.level_table(R.CONFIGS["tiny"]), R.table("tiny")
    x = R.points("tiny", set_name)[:64]
    for active in (None, 2):
        fast, _ = R.encode(torch.tensor(x).double(), torch.tensor(P).double(), levels, active)
        slow = R.encode_slow(x, P, levels, active)
        assert np.array_equal(np.isnan(fast.numpy()), np.isnan(slow))
        np.testing.assert_allclose(np.nan_to_num(fast.numpy()), np.nan_to_num(slow), rtol=0, atol=1e-14)
        if active:
            assert not fast.numpy()[:, 2 * active:][~np.isnan(slow[:, 0])].any()
    if set_name == "outside":
        assert np.isnan(slow[5]).all() and np.isfinite(np.delete(slow, 5, axis=0)).all()


def test_x_of_one_aliases_into_the_next_row_of_a_dense_level():
    lv = R.level_table(R.CONFIGS["tiny"])[1]                                    # resolution 4, 64 entries, dense, scale 3
    cell = torch.floor(torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64) * lv.scale + 0.5).to(torch.int64)
    assert cell.tolist() == [[3, 0, 0]]
    idx = R.corner_indices(cell, lv)[0].tolist()
    assert idx[0] == 3 and idx[1] == 4                                          # corner coordinate 4 = res: entry (0, 1, 0), the next row's first
    assert idx[1] == R.corner_indices(torch.tensor([[0, 1, 0]]), lv)[0, 0].item()
    top = R.corner_indices(torch.tensor([[3, 3, 3]]), lv)[0].tolist()           # the far corner of the cube: the index wraps % size
    assert top[7] == (4 + 4 * 4 + 4 * 16) % 64 and all(0 <= i < 64 for i in top)
    far = R.corner_indices(torch.tensor([[-1, -7, 12345678]]), R.level_table(R.CONFIGS["tiny"])[3])
    assert ((far >= 0) & (far < 64)).all()


@pytest.mark.parametrize("config_name,set_name", R.CASES)
def test_the_kink_cap(config_name, set_name):
    c = R.case(config_name, set_name)
    n = int(c["kinks"].sum())
    print(f"{config_name}/{set_name}: {n} of {len(c['x'])} points on a ReLU kink")
    assert n <= R.KINK_CAP * len(c["x"])
    # and the rule's noise model holds where it is meant to: with the float64 run's encoding rounded to fp32 (what a kernel that forms enc in double
    # holds in its registers), an fp32 product W1 enc flips the sign of no hidden unit on the points that stay
    W1 = torch.tensor(c["W1"])
    _, enc, z64, _ = R.field(torch.tensor(c["xb"]), torch.tensor(c["params"]).double(), c["levels"], W1.double(), torch.tensor(c["W2"]).double(), R.BBOX)
    keep = ~c["kinks"] & c["valid_b"]
    z32 = enc[keep].float() @ W1.T
    assert ((z64[keep] > 0) == (z32 > 0)).all()


def test_gradcheck_of_the_restatement():
    levels = R.level_table(R.CONFIGS["tiny"])
    x = torch.tensor(R.points("tiny", "uniform")[:6]).double().requires_grad_(True)
    P = torch.tensor(R.table("tiny")).double().requires_grad_(True)
    W1, W2 = (torch.tensor(w).double().requires_grad_(True) for w in R.weights("tiny"))
    assert torch.autograd.gradcheck(lambda a, b: R.encode(a, b, levels)[0], (x, P), eps=1e-7, atol=1e-6)
    x32 = torch.tensor(R.unbox(R.points("tiny", "uniform")[:6]))
    assert torch.autograd.gradcheck(lambda p, a, b: R.field(x32, p, levels, a, b, R.BBOX, 0.25)[0], (P, W1, W2), eps=1e-7, atol=1e-6)


def test_the_cases_are_what_the_issue_lists():
    assert set(R.CASES) == {("default", "uniform"), ("default", "pile")} | {(c, s) for c in ("tiny", "odd") for s in R.POINT_SETS}
    assert len(R.points("tiny", "uniform")) == 4099 and len(R.points("odd", "pile")) == 4096 and len(R.points("tiny", "one")) == 1
    lattice = R.points("odd", "lattice")
    assert {tuple(r) for r in lattice[:8].tolist()} == {(a, b, c) for a in (0.0, 1.0) for b in (0.0, 1.0) for c in (0.0, 1.0)}
    out = R.points("tiny", "outside")
    assert np.isnan(out).any(axis=1).sum() == 1 and np.nanmin(out) >= -0.5 and np.nanmax(out) <= 1.5 and (np.nanmin(out) < 0 or np.nanmax(out) > 1)
    c = R.case("tiny", "pile")
    assert c["enc"]["n"] >= 4096
    g = R.upstream("one_row", (9, 4), "x")
    assert (np.abs(g).sum(axis=1) > 0).sum() == 1
