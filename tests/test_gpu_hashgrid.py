"""GPU: youreditableavatar_amd.hashgrid (csrc/tgs_hashgrid.hip) against the rules as tests/hashgrid_ref.py restates them in torch float64.

Every value follows the project's bars (tests/mesh_grad_ref.py's ``check_bars``): max |got - ref64| <= 4 eta (+ the fixed-point term for dL_dparams), with
eta = max |ref32 - ref64| of the same restatement in float32 on the float64 run's cells; rel-L2 <= 4x ref32's; exact zeros where the reference's rows are
zero.  The fixed-point term is the header's n 2^(e-35) with B restated from the inputs (max |dL_denc| on the encode path, the analytic bound on the fused
path) and n the largest number of contributions to one entry of the case.  Points on a ReLU kink (tests/test_hashgrid_ref.py caps their number) carry a zero
upstream.  The NaN row of ``outside`` is compared apart.  Every backward runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import youreditableavatar_amd.hashgrid as hg
from tests import hashgrid_ref as R
from tests.mesh_grad_ref import check_bars, fixed_point_term

pytestmark = pytest.mark.gpu
ONE_ROW = [("tiny", "uniform"), ("odd", "uniform")]
BIAS = 0.25


def _dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def _levels(config_name, c):
    levels = hg.level_table(R.CONFIGS[config_name])
    assert [tuple(v) for v in levels] == [tuple(v) for v in c["levels"]]
    return levels


def run_encode(c, levels):
    x, P = _dev(c["x"], True), _dev(c["params"], True)
    enc = hg.hashgrid_encode(x, P, levels, c["active"])
    enc.backward(_dev(c["g_enc"]))
    return enc.detach(), P.grad, x.grad


def run_field(c, levels):
    P, W1, W2 = _dev(c["params"], True), _dev(c["W1"], True), _dev(c["W2"], True)
    out = hg.sdf_field(_dev(c["xb"]), P, levels, W1, W2, bbox=R.BBOX, bias=BIAS, active_levels=c["active"])
    out.backward(_dev(c["g_out"]))
    return out.detach(), P.grad, W1.grad, W2.grad


def check_encode(c, got, tag):
    enc, d_p, d_x = got
    v, ref = c["valid"], c["enc"]
    r64, r32 = ref["ref64"], ref["ref32"]
    check_bars(tag + " enc", _np(enc)[v], r64["enc"][v], r32["enc"][v])
    check_bars(tag + " dL_dparams", _np(d_p).reshape(-1, 2), r64["d_params"].reshape(-1, 2), r32["d_params"].reshape(-1, 2), fixed_point_term(ref["B"], ref["n"]))
    check_bars(tag + " dL_dx", _np(d_x)[v], r64["d_x"][v], r32["d_x"][v])
    assert torch.isnan(enc[~torch.from_numpy(v)]).all() and torch.isnan(d_x[~torch.from_numpy(v)]).all()      # the NaN row: NaN forward, NaN dL_dx


def check_field(c, got, tag):
    out, d_p, d_w1, d_w2 = got
    v, ref = c["valid_b"], c["fld"]
    r64, r32 = ref["ref64"], ref["ref32"]
    check_bars(tag + " out", _np(out)[v], r64["out"][v], r32["out"][v])
    check_bars(tag + " dL_dparams", _np(d_p).reshape(-1, 2), r64["d_params"].reshape(-1, 2), r32["d_params"].reshape(-1, 2), fixed_point_term(ref["B"], ref["n"]))
    check_bars(tag + " dL_dW1", _np(d_w1), r64["d_W1"], r32["d_W1"])
    check_bars(tag + " dL_dW2", _np(d_w2), r64["d_W2"], r32["d_W2"])
    assert torch.isnan(out[~torch.from_numpy(v)]).all()


@pytest.mark.parametrize("config_name,set_name", R.CASES)
def test_the_encoding_and_its_two_gradients(config_name, set_name):
    c = R.case(config_name, set_name)
    levels = _levels(config_name, c)
    first, again = run_encode(c, levels), run_encode(c, levels)
    check_encode(c, first, f"{config_name}/{set_name}")
    for a, b in zip(first, again):
        assert _same_bits(a, b)


@pytest.mark.parametrize("config_name,set_name", R.CASES)
def test_the_fused_field_and_its_three_gradients(config_name, set_name):
    c = R.case(config_name, set_name)
    levels = _levels(config_name, c)
    first, again = run_field(c, levels), run_field(c, levels)
    check_field(c, first, f"{config_name}/{set_name}")
    for a, b in zip(first, again):
        assert _same_bits(a, b)


@pytest.mark.parametrize("config_name,set_name", ONE_ROW)
def test_a_single_upstream_row(config_name, set_name):
    c = R.case(config_name, set_name, "one_row")
    levels = _levels(config_name, c)
    check_encode(c, run_encode(c, levels), f"{config_name}/{set_name}/one_row")
    check_field(c, run_field(c, levels), f"{config_name}/{set_name}/one_row")


@pytest.mark.parametrize("config_name", ["tiny", "odd"])
def test_the_levels_above_active_levels_are_exact_zeros(config_name):
    active = R.CONFIGS[config_name]["n_levels"] // 2
    c = R.case(config_name, "uniform", "random", active)
    levels = _levels(config_name, c)
    enc, d_p, d_x = got = run_encode(c, levels)
    assert not enc[:, 2 * active:].any() and enc[:, :2 * active].any()
    assert not d_p[2 * levels[active].offset:].any() and d_p[:2 * levels[active].offset].any()
    check_encode(c, got, f"{config_name}/active={active}")
    out, f_p, f_w1, f_w2 = fgot = run_field(c, levels)
    assert not f_p[2 * levels[active].offset:].any() and not f_w1[:, 2 * active:].any()
    check_field(c, fgot, f"{config_name}/active={active}")
    c0 = R.case(config_name, "one")
    x, P = _dev(c0["x"]), _dev(c0["params"], True)                               # no level at all: zeros everywhere
    none = hg.hashgrid_encode(x, P, levels, 0)
    none.backward(torch.ones_like(none))
    assert not none.any() and not P.grad.any()


@pytest.mark.parametrize("config_name", ["tiny", "odd"])
def test_the_nan_row_leaves_the_other_rows_alone(config_name):
    c = R.case(config_name, "outside")
    levels = _levels(config_name, c)
    assert (~c["valid"]).sum() == 1 and (~c["valid_b"]).sum() == 1
    keep = torch.from_numpy(c["valid"]).cuda()
    x, xb, P, W1, W2 = (_dev(c[k]) for k in ("x", "xb", "params", "W1", "W2"))
    enc, short = hg.hashgrid_encode(x, P, levels), hg.hashgrid_encode(x[keep], P, levels)
    assert torch.isnan(enc[~keep]).all() and torch.isfinite(short).all() and torch.equal(enc[keep], short)
    out, fshort = hg.sdf_field(xb, P, levels, W1, W2, R.BBOX, BIAS), hg.sdf_field(xb[keep], P, levels, W1, W2, R.BBOX, BIAS)
    assert torch.isnan(out[~keep]).all() and torch.isfinite(fshort).all() and torch.equal(out[keep], fshort)
    _, d_p, d_x = run_encode(c, levels)                                           # (their values: test_the_encoding_and_its_two_gradients)
    assert torch.isfinite(d_p).all() and torch.isnan(d_x[~keep]).all() and torch.isfinite(d_x[keep]).all()
    assert all(torch.isfinite(t).all() for t in run_field(c, levels)[1:])
    huge = torch.tensor([[0.5, 2000.0, 0.5], [0.5, 0.5, float("inf")]]).cuda()   # beyond 1024, and an infinity: NaN rows too
    assert torch.isnan(hg.hashgrid_encode(huge, P, levels)).all()
    g = _dev(c["g_enc"]).clone()
    g[3, 1] = float("nan")                                                       # a non-finite bound: the whole gradient is NaN
    P2 = _dev(c["params"], True)
    hg.hashgrid_encode(x, P2, levels).backward(g)
    assert torch.isnan(P2.grad).all()


def test_the_module_the_fused_path_and_the_fallback():
    grid = hg.HashGrid(3, R.CONFIGS["default"])
    assert grid.params.numel() == 12196240 and grid.n_output_dims == 32 and grid.n_input_dims == 3
    c = R.case("odd", "uniform")
    grid = hg.HashGrid(3, R.CONFIGS["odd"]).cuda()
    with torch.no_grad():
        grid.params.copy_(_dev(c["params"]))
    xb, mn, mx = _dev(c["xb"]), torch.tensor(R.BBOX[0]).cuda(), torch.tensor(R.BBOX[1]).cuda()
    fused = hg.SdfField(grid, _dev(c["W1"]), _dev(c["W2"]), bbox=R.BBOX, bias=BIAS)
    assert fused.fused
    # hashgrid_encode plus the torch layers: the same values within the same bars, with its gradients
    P, W1, W2 = _dev(c["params"], True), _dev(c["W1"], True), _dev(c["W2"], True)
    out = torch.relu(hg.hashgrid_encode((xb - mn) / (mx - mn), P, grid.levels) @ W1.T) @ W2.T + BIAS
    out.backward(_dev(c["g_out"]))
    check_field(c, (out.detach(), P.grad, W1.grad, W2.grad), "odd/uniform unfused")
    got = fused(xb)
    got.backward(_dev(c["g_out"]))
    check_field(c, (got.detach(), grid.params.grad, fused.W1.grad, fused.W2.grad), "odd/uniform SdfField")
    # a network the kernel does not cover goes through the encoding and the torch layers
    torch.manual_seed(5)
    lin = lambda i, o: torch.nn.Linear(i, o, bias=False)
    net = torch.nn.Sequential(lin(10, 64), torch.nn.ReLU(), lin(64, 64), torch.nn.ReLU(), lin(64, 1)).cuda()
    deep = hg.SdfField(grid, net, bbox=R.BBOX, bias=BIAS)
    assert not deep.fused
    grid.params.grad = None
    val = deep(xb, 3)
    want = net(grid((xb - mn) / (mx - mn), 3)) + BIAS
    assert torch.equal(val, want) and tuple(val.shape) == (len(xb), 1)
    val.sum().backward()
    assert grid.params.grad is not None and grid.params.grad.any() and net[0].weight.grad.any()
    assert not grid.params.grad[2 * grid.levels[3].offset:].any()
    # a network it covers is fused, on its own weights
    small = torch.nn.Sequential(lin(10, 32), torch.nn.ReLU(inplace=True), lin(32, 2)).cuda()
    f2 = hg.SdfField(grid, small)
    assert f2.fused and f2.W1 is small[0].weight
    unit = (xb - mn) / (mx - mn)
    a, b = f2(unit), small(grid(unit))
    # two fp32 evaluations of sums of 10 and 32 products: each is within (10 + 32) 2^-24 of the sum of the products' magnitudes, whatever its order
    terms = (grid(unit).abs() @ small[0].weight.abs().T) @ small[2].weight.abs().T
    assert ((a - b).abs() <= 2 * 42 * 2.0 ** -24 * terms).all()
    a.sum().backward()
    assert small[0].weight.grad.any() and small[2].weight.grad.any()
    with pytest.raises(RuntimeError, match="no gradient with respect to x"):
        f2(unit.clone().requires_grad_(True)).sum().backward()


def test_no_points_and_no_second_derivative():
    c = R.case("tiny", "one")
    levels = _levels("tiny", c)
    P, W1, W2 = _dev(c["params"], True), _dev(c["W1"], True), _dev(c["W2"], True)
    x0 = torch.zeros((0, 3), device="cuda", requires_grad=True)
    enc = hg.hashgrid_encode(x0, P, levels)
    assert tuple(enc.shape) == (0, 8)
    out = hg.sdf_field(x0.detach(), P, levels, W1, W2)
    assert tuple(out.shape) == (0, 3)
    (enc.sum() + out.sum()).backward()
    for t in (P, W1, W2):
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()
    assert tuple(x0.grad.shape) == (0, 3)
    x = _dev(c["x"], True)
    w = torch.ones(8, device="cuda", requires_grad=True)                          # (the analytic normal's case: the upstream depends on the network's weights)
    (d_x,) = torch.autograd.grad((hg.hashgrid_encode(x, P, levels) * w).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        d_x.sum().backward()
    only_p = hg.hashgrid_encode(x.detach(), P, levels)                            # dL_dx is computed only where x requires it
    P.grad = None
    only_p.sum().backward()
    assert P.grad.any()
