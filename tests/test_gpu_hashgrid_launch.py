"""GPU: the hash-grid kernels (csrc/tgs_hashgrid.hip) at the launch shapes tests/test_gpu_hashgrid.py never reaches: ``R.LAUNCH_CASES``.

  many   262 733 points: more tiles than k_hg_field_bwd has workgroups, so workgroups 0, 1 and 2 loop (a1/a2 carried, the barrier between tiles, the
         partial tile on a second trip) and k_hg_field_reduce adds 1024 slabs.
  runs   runs of every length in one cell, per level another: WaveRuns.merged with mixed ``end``, runs across waves and workgroups, a NaN row inside a
         run, and one inside a run that truly lies in cell (0,0,0), which is what an invalid lane's zeroed HgCell holds.
  far    |x| up to 1024 exactly, the next float above it, -inf: negative cells that wrap as uint32 on dense and hashed levels.
  wide, wide_thin, single, single_wide: H64 D4 (every a1/a2 slot, o2 == 3), 16 levels under H16 (the chunk loop's break), C = 2 and D = 2.

Two kinds of bars.  The project's (``check_bars``, as tests/test_gpu_hashgrid.py applies them) on every case but ``far``, where the float32 restatement
loses ``frac`` and eta says nothing.  And the round-once bars of ``check_round_once`` on the encode path of every case, ``far`` included: they follow from
the header's rules and from nothing that was measured.  Every backward runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import youreditableavatar_amd.hashgrid as hg
from tests import hashgrid_ref as R
from tests.mesh_grad_ref import check_bars, fixed_point_term
from tests.test_gpu_hashgrid import BIAS, _dev, _levels, _np, _same_bits, check_encode, check_field, run_encode, run_field

pytestmark = pytest.mark.gpu
U64, U32 = 2.0 ** -53, 2.0 ** -24                                         # the unit roundoffs
TINY32 = 2.0 ** -150                                                      # half the spacing of float32's denormals: what one rounding costs below 2^-126


def gamma(n, u=U64):
    """n roundings of relative size u compound to at most n u / (1 - n u)"""
    return n * u / (1.0 - n * u)


def check_round_once(c, m, got, tag):
    """The header: enc and dL_dx are "formed in double and rounded once", dL_dparams is fixed point plus one convert rounding.  Against the float64
    restatement, element by element:

        |enc - ref64|        <= 2^-24 |ref64| + d        d   = gamma(28) M_enc
        |dL_dx - ref64|      <= 2^-24 |ref64| + d_x      d_x = gamma(2 (16 + L) + 2) M_x
        |dL_dparams - ref64| <= 2^-24 |ref64| + fixed_point_term(B, n) + d_p      d_p = gamma(14 + n_e) M_p

    (each + 2^-150: one rounding to float32 costs half a denormal's spacing where the value lies below 2^-126).  M are ``R.term_sums``: the sums of the
    magnitudes of the terms, gamma(k) = k 2^-53 / (1 - k 2^-53).  pos = x scale + 0.5 is the SAME double on both sides (the product of two float32 is
    exact in double, the sum rounds once under IEEE, fused or not), so cell and frac = pos - cell (exact) carry no difference; that is what lets the
    bars hold at |x| = 1024, where float32 has lost frac.  The counts of roundings between the exact value of the terms and a side's double:
      enc    a weight is three factors frac or 1 - frac (<= 1 rounding each) and two products: 5; times the row: 6; the sum of 8 terms in any order: 7.
             13 a side, 26 for the two, + 1 because the kernel rounds ITS double (within d of ref64) to float32, + 1 of slack: 28.
      dL_dx  s = g_0 row_0 + g_1 row_1: 3; the two other weights and their product: 3; the product with s: 1; the 8 corners: 7; times the scale: 1;
             the L levels: L - 1; autograd's chain has the same operations in another order.  <= 16 + L a side, + 2 as above.
      dL_dparams  kernel: the weight 5, times g 1, the power-of-two scale exact, the integer sum exact, the accumulator to double 1: 7 (the rounding to
             fixed point is the fixed-point term, the convert's rounding the 2^-24 term).  Restatement: the weight 5, times g 1, the n_e contributions
             of the element in any order n_e - 1.  12 + n_e for the two, + 2 as above; n_e <= n, the case's largest count, is used for every element.
    The figures are printed before they are asserted; the bars are not set from them."""
    enc, d_p, d_x = (_np(t).astype(np.float64) for t in got)
    v, ref = c["valid"], c["enc"]
    r64 = ref["ref64"]
    L = len(c["levels"])
    bars = {
        "enc": (enc[v], r64["enc"][v], gamma(28) * m["enc"][v]),
        "dL_dx": (d_x[v], r64["d_x"][v], gamma(2 * (16 + L) + 2) * m["d_x"][v]),
        "dL_dparams": (d_p, r64["d_params"], fixed_point_term(ref["B"], ref["n"]) + gamma(14 + ref["n"]) * m["d_params"]),
    }
    worst = {}
    for name, (a, r, d) in bars.items():
        assert np.isfinite(a).all() and np.isfinite(r).all(), (tag, name)
        err, bar = np.abs(a - r), U32 * np.abs(r) + d + TINY32
        at = int(np.argmax(err / bar)) if err.size else 0
        worst[name] = float((err / bar).max()) if err.size else 0.0
        print(f"{tag} round-once {name}: max err {float(err.max()):.3g}, largest err/bar {worst[name]:.3g} (err {err.flat[at]:.3g}, bar {bar.flat[at]:.3g}, "
              f"of which 2^-24 |ref| {U32 * abs(r.flat[at]):.3g} and the double and fixed-point terms {np.broadcast_to(d, r.shape).flat[at]:.3g})")
    for name, ratio in worst.items():
        assert ratio <= 1.0, (tag, name, ratio)
    bad = torch.from_numpy(~v)
    assert torch.isnan(got[0][bad]).all() and torch.isnan(got[2][bad]).all()                                      # the NaN rows: NaN forward, NaN dL_dx


def _permutation(n):
    return np.random.default_rng(1717).permutation(n)


# ---- every launch case: the encoding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config_name,set_name", R.LAUNCH_CASES)
def test_the_encoding_at_the_launch_shapes(config_name, set_name):
    c = R.case(config_name, set_name)
    levels = _levels(config_name, c)
    tag = f"{config_name}/{set_name}"
    first, again = run_encode(c, levels), run_encode(c, levels)
    for a, b in zip(first, again):
        assert _same_bits(a, b)
    if set_name != "far":                                                        # (far: eta of the float32 restatement is vacuous)
        check_encode(c, first, tag)
    check_round_once(c, R.magnitudes(config_name, set_name), first, tag)
    if set_name == "far":
        assert c["valid"][-3] and not c["valid"][-2] and not c["valid"][-1] and torch.isfinite(first[0][-3]).all() and first[0][-3].any()
    if set_name == "runs":                                                       # integer sums commute: any order of the points gives the same bits
        perm = _permutation(len(c["x"]))
        _, p_p, p_x = run_encode(dict(c, x=c["x"][perm], g_enc=c["g_enc"][perm]), levels)
        assert _same_bits(p_p, first[1])
        assert _same_bits(p_x, first[2][torch.from_numpy(perm).cuda()])


# ---- every launch case: the fused field ----------------------------------------------------------------------------------------------
def _far_forward(c, out, tag):
    """``far``, the fused forward alone, against the float64 restatement under the fp32-product bound of test_the_module_the_fused_path_and_the_fallback:
    one fp32 evaluation of sums of C and H products is within (C + H) 2^-24 (compounded: gamma) of the sum of the products' magnitudes T, whatever its
    order; the final + bias rounds once more, 2^-24 |out|; and the encoding the products start from is the float64 one rounded once, |d enc| <=
    2^-24 |enc| + gamma(28) M_enc, which reaches the output through |W1| and |W2| (relu is 1-Lipschitz, so a kink adds nothing here)."""
    v = c["valid_b"]
    W1, W2 = torch.tensor(c["W1"]).double(), torch.tensor(c["W2"]).double()
    ref, enc, _, _ = R.field(torch.tensor(c["xb"]), torch.tensor(c["params"]).double(), c["levels"], W1, W2, R.BBOX, BIAS)
    xm = R.box_map(torch.tensor(c["xb"]), R.BBOX)
    m = R.term_sums(xm.numpy(), v, c["params"], np.zeros((len(v), enc.shape[1]), np.float32), c["levels"])
    enc = torch.nan_to_num(enc.abs(), nan=0.0)
    d_enc = U32 * enc + gamma(28) * torch.from_numpy(m["enc"]) + TINY32
    H, C = W1.shape
    through = lambda e: (e @ W1.abs().T) @ W2.abs().T
    bar = (gamma(C + H, U32) * through(enc + d_enc) + U32 * ref.abs() + through(d_enc)).numpy()[v]
    err = np.abs(_np(out).astype(np.float64) - ref.numpy())[v]
    print(f"{tag} fused out against the fp32-product bound: max err {err.max():.3g}, largest err/bar {(err / bar).max():.3g}, smallest bar {bar.min():.3g}")
    assert np.isfinite(err).all() and (err <= bar).all()
    assert torch.isnan(out[~torch.from_numpy(v)]).all() and (~v).sum() >= 2


@pytest.mark.parametrize("config_name,set_name", R.LAUNCH_CASES)
def test_the_fused_field_at_the_launch_shapes(config_name, set_name):
    """On ``far`` the fused backward's VALUES are not compared: eta of the float32 restatement is vacuous there (it loses frac at large pos: eta of dL_dx
    up to 0.57), and no derived bar is attempted for fp32 products behind a ReLU.  What is checked there: the forward under the fp32-product bound,
    finite gradients, NaN rows that contribute nothing, and two runs with the same bits."""
    c = R.case(config_name, set_name)
    levels = _levels(config_name, c)
    tag = f"{config_name}/{set_name}"
    first, again = run_field(c, levels), run_field(c, levels)
    for a, b in zip(first, again):
        assert _same_bits(a, b)
    if set_name != "far":
        check_field(c, first, tag)
    else:
        _far_forward(c, first[0], tag)
        assert all(torch.isfinite(t).all() and t.any() for t in first[1:])
        # the NaN rows contribute nothing: the same bits with an in-range point and a zero upstream in their place (the other points keep their tiles)
        bad = ~c["valid_b"]
        xb, g = c["xb"].copy(), c["g_out"].copy()
        assert np.abs(g[bad]).min() > 0.0
        xb[bad], g[bad] = R.unbox(np.full((1, 3), 0.375, np.float32)), 0.0
        assert np.frexp(R.field_bound(g, c["W1"], c["W2"]))[1] == np.frexp(c["fld"]["B"])[1]                     # (the same fixed-point exponent)
        without = run_field(dict(c, xb=xb, g_out=g), levels)
        assert torch.isfinite(without[0]).all()
        for a, b in zip(first[1:], without[1:]):
            assert _same_bits(a, b)
    if set_name == "many":
        few = 4099                                                               # (the 17 tiles of the one-trip cases)
        head = hg.sdf_field(_dev(c["xb"][:few]), _dev(c["params"]), levels, _dev(c["W1"]), _dev(c["W2"]), bbox=R.BBOX, bias=BIAS)
        assert torch.isfinite(head).all() and _same_bits(first[0][:few], head)
        r64 = c["fld"]["ref64"]
        assert ((_np(first[2]) != 0).any(axis=0) == (r64["d_W1"] != 0).any(axis=0)).all() and (r64["d_W1"] != 0).any(axis=0).all()
        assert ((_np(first[3]) != 0).any(axis=1) == (r64["d_W2"] != 0).any(axis=1)).all() and (r64["d_W2"] != 0).any(axis=1).all()
    if set_name == "runs":
        perm = _permutation(len(c["x"]))
        p_out, p_p, p_w1, p_w2 = run_field(dict(c, xb=c["xb"][perm], g_out=c["g_out"][perm]), levels)
        assert _same_bits(p_out, first[0][torch.from_numpy(perm).cuda()])
        assert _same_bits(p_p, first[1])                                         # (dL_dW1 and dL_dW2 are float sums in the points' order: the bars only)
        r64, r32 = c["fld"]["ref64"], c["fld"]["ref32"]
        check_bars(tag + " permuted dL_dW1", _np(p_w1), r64["d_W1"], r32["d_W1"])
        check_bars(tag + " permuted dL_dW2", _np(p_w2), r64["d_W2"], r32["d_W2"])


# ---- an all-zero upstream --------------------------------------------------------------------------------------------------------------
def test_a_zero_upstream_stores_exact_zeros_over_garbage():
    """max |g| = 0: grad_scale is false and nothing is accumulated; every gradient must still be STORED.  Through the C ABI, so that the outputs and
    the workspace can hold garbage (NaN bits) before the call."""
    c = R.case("tiny", "uniform")
    levels = tuple(_levels("tiny", c))
    x, xb, P, W1, W2 = (_dev(c[k]) for k in ("x", "xb", "params", "W1", "W2"))
    N, dev = len(c["x"]), x.device
    H, D = R.MLP["tiny"]
    junk = lambda *shape: torch.full(shape, float("nan"), device=dev)

    d_p, d_x, g = junk(P.numel()), junk(N, 3), torch.zeros((N, 2 * len(levels)), device=dev)
    ws, nbytes = hg._workspace(P.numel(), 0, 0, dev)
    ws.fill_(0xFF)
    recs, head = hg._head(dev, N, x, P, levels, len(levels))
    hg._ok(hg._lib.tgs_hashgrid_encode_backward(*head, g.data_ptr(), d_p.data_ptr(), d_x.data_ptr(), ws.data_ptr(), nbytes))
    assert torch.equal(d_p, torch.zeros_like(d_p)) and torch.equal(d_x, torch.zeros_like(d_x))

    f_p, f_w1, f_w2, g = junk(P.numel()), junk(H, 2 * len(levels)), junk(D, H), torch.zeros((N, D), device=dev)
    ws, nbytes = hg._workspace(P.numel(), H, D, dev)
    ws.fill_(0xFF)
    recs, head = hg._head(dev, N, xb, P, levels, len(levels))
    box, tail = hg._field_tail(hg._check_bbox(R.BBOX), W1, W2, H, D)
    hg._ok(hg._lib.tgs_hashgrid_field_backward(*head, *tail, g.data_ptr(), f_p.data_ptr(), f_w1.data_ptr(), f_w2.data_ptr(), ws.data_ptr(), nbytes))
    for t in (f_p, f_w1, f_w2):
        assert torch.equal(t, torch.zeros_like(t))
    zero = dict(c, g_enc=np.zeros_like(c["g_enc"]), g_out=np.zeros_like(c["g_out"]))                              # and through autograd
    for t in run_encode(zero, levels)[1:] + run_field(zero, levels)[1:]:
        assert torch.equal(t, torch.zeros_like(t))


# ---- an upstream over many binades -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binades", "denormal"])
def test_the_dynamic_range_of_the_upstream(kind):
    """binades: one row of the upstream is 2^40 above the others, whose contributions the bound's exponent leaves few fixed-point bits.  denormal:
    max |g| = 2^-130, the bound itself is a denormal float.  The same bars, with B restated from the inputs."""
    c = R.case("tiny", "uniform", kind)
    levels = _levels("tiny", c)
    tag = f"tiny/uniform/{kind}"
    big = np.abs(c["g_enc"]).max()
    assert big == 2.0 ** -130 if kind == "denormal" else (big > 2.0 ** 19 and np.median(np.abs(c["g_enc"])) < 2.0 ** -20)
    got, fgot = run_encode(c, levels), run_field(c, levels)
    assert all(torch.isfinite(t).all() and t.any() for t in got + fgot)
    check_encode(c, got, tag)
    check_round_once(c, R.magnitudes("tiny", "uniform", kind), got, tag)
    check_field(c, fgot, tag)


# ---- the Python wrapper on tensors that are not contiguous -------------------------------------------------------------------------------
def test_the_wrapper_on_strided_tensors():
    c = R.case("odd", "uniform")
    levels = _levels("odd", c)
    N, (H, D), C = len(c["x"]), R.MLP["odd"], 2 * len(levels)
    x4 = torch.cat([_dev(c["x"]), torch.full((N, 1), 9.0, device="cuda")], dim=1)
    g2 = torch.stack([_dev(c["g_enc"]), torch.full((N, C), 5.0, device="cuda")], dim=2)                           # [N,C,2]: g is every other float
    xs, gs = x4[:, :3].detach().requires_grad_(True), g2[:, :, 0]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    P = _dev(c["params"], True)
    enc = hg.hashgrid_encode(xs, P, levels)
    enc.backward(gs)
    want = run_encode(c, levels)
    for a, b in zip((enc.detach(), P.grad, xs.grad), want):
        assert _same_bits(a, b)

    xb4 = torch.cat([torch.full((N, 1), -9.0, device="cuda"), _dev(c["xb"])], dim=1)
    W1t = _dev(c["W1"]).T.contiguous()                                                                            # [C,H]
    W1s, xbs = W1t.T.detach().requires_grad_(True), xb4[:, 1:]
    gcol = _dev(c["g_out"])[:, :1]
    ge = gcol.expand(N, D)                                                                                        # stride (D, 0)
    assert not W1s.is_contiguous() and not xbs.is_contiguous() and not ge.is_contiguous() and tuple(W1s.shape) == (H, C)
    P, W2 = _dev(c["params"], True), _dev(c["W2"], True)
    out = hg.sdf_field(xbs, P, levels, W1s, W2, bbox=R.BBOX, bias=BIAS)
    out.backward(ge)
    want = run_field(dict(c, g_out=_np(ge.contiguous())), levels)
    for a, b in zip((out.detach(), P.grad, W1s.grad, W2.grad), want):
        assert _same_bits(a, b)
    assert W1s.grad.any() and W2.grad.any() and P.grad.any()
