"""The fused SH -> RGB kernels (csrc/tgs_shcolor.hip: k_sh_rgb, k_sh_rgb_dcrest; youreditableavatar_amd/sh_color.py) row by row on every
staging path, against oracle/sh_color_ref.points_rgb evaluated in float64 with autograd (dc / rest and groups: the same function on torch.cat).

Two tiers per case, forward and backward, camera mode and direction mode:
  1. whole tensors: util.rel_l2 <= 1e-6 for the colours and the SH gradients, <= 1e-5 for the position / direction gradients (the numbers of
     tests/test_gpu_api.py for this op);
  2. every row against a scale that cancellation cannot shrink, in float64 from the reference (oracle/sh_color_ref.row_scales; B_k = basis of
     the row's direction, dRGB = upstream gradient where the colour before the clamp is >= 0, else 0; u = 2^-24):
       colours                         |x - ref| <= 32 u (0.5 + sum_k |B_k| |sh_kc|)                       per element
       SH gradient (dc and rest)       row norm of the error <= 32 u x row norm of |B_k| |dRGB_c|; rows with all three channels clamped and
                                       every coefficient above the active levels exactly 0
       position / direction gradient   row norm of the error <= 128 u ||A|| / max(|v|, 1e-12), A_j = sum_c |dRGB_c| sum_k |dB_k/dd_j| |sh_kc|,
                                       |v| the distance to the camera (1 in direction mode); exactly 0 at one level.
                                       [Pe,1] positions (the sum of the three components): sqrt(3) (128 + 2) u ||A|| / |v|, see row_distances.
     The factors are first-order rounding bounds: a colour is a 16-term dot product over a basis of <= 6 operations behind a 5-operation
     normalisation (gamma_32); the direction gradient sums 45 products and passes a projection and a division (gamma_128).
     test_fp32_restatement_is_within_the_row_bars shows without the code under test that fp32 arithmetic reaches them.
Rows whose colour before the clamp lies within the colour bar of zero in float64 are undecidable (the kernel may clamp the other way): they
are left out of the gradient comparisons only, and a case may lose at most 1e-4 of its rows that way (asserted on the CPU for every case).

The cases: every valid (M, levels) of points_rgb and a sweep of P over the workgroup boundaries; for points_rgb_dc_rest the three data paths
of the kernel (oracle/sh_color_ref.dcrest_path) each with one workgroup, several full workgroups and a ragged last workgroup --
test_dcrest_cases_cover_every_path proves it from the table; the two-group entry point; the same bits from both entry points and from two runs;
edge rows; the stores through the C ABI into canary-framed buffers; views that are 4-byte but not 16-byte aligned.

A row whose colour before the clamp is EXACTLY 0 in both precisions cannot be constructed: the kernel multiplies by the fp32 roundings of the
SH constants and the reference by their doubles, so the two sums differ by ~1e-8 of their terms whatever the inputs.  The edge case holds the
nearest thing -- one level, dc chosen so that the fp32 product is exactly -0.5 -- where the reference is ~1e-8 from zero: an undecidable row
by the rule above, checked for its colour only.
"""
import numpy as np
import pytest
import torch

from oracle import sh_color_ref as R
from tests import util

CAM = (0.3, -2.0, 1.5)
WHOLE_TOL = {"colors": 1e-6, "dsh": 1e-6, "dvec": 1e-5}
MAX_EXCLUDED_SHARE = 1e-4
CANARY = -7.75
P_SWEEP = (1, 255, 256, 257, 1001, 100_000, 500_000)


def _valid_levels(M):
    return [l for l in (1, 2, 3, 4) if l * l <= M]


# points_rgb / k_sh_rgb: (M, levels, P)
RGB_CASES = sorted(set([(M, l, P) for M in (1, 4, 9, 12, 16) for l in _valid_levels(M) for P in (257, 100_000)] +
                       [(M, l, P) for (M, l) in ((16, 4), (9, 2)) for P in P_SWEEP]))

# points_rgb_dc_rest / k_sh_rgb_dcrest: (Mr, levels, P, aligned rest).  P from {1, 4, 256, 257, 260, 1000, 1001, 1024, 100 000, 100 001, 500 000}
DCREST_CASES = [
    (0, 1, 257, True), (0, 1, 100_000, True),
    (3, 1, 1001, True), (3, 2, 4, True), (3, 2, 1024, True), (3, 2, 1000, True), (3, 2, 1001, True), (3, 2, 1, True),
    (5, 1, 257, True), (5, 2, 256, True), (5, 2, 1024, True), (5, 2, 260, True), (5, 2, 257, True),
    (8, 1, 1000, True), (8, 2, 257, True), (8, 2, 100_001, True), (8, 3, 1, True), (8, 3, 1001, True), (8, 3, 1024, True), (8, 3, 100_000, True),
    (14, 1, 260, True), (14, 2, 1000, True), (14, 2, 1001, True), (14, 3, 100_000, True), (14, 3, 257, True), (14, 3, 1024, True),
    (15, 1, 257, True), (15, 1, 500_000, True), (15, 2, 1024, True), (15, 2, 100_000, True), (15, 2, 100_001, True),
    (15, 3, 4, True), (15, 3, 260, True), (15, 3, 1001, True),
    (15, 4, 1, True), (15, 4, 4, True), (15, 4, 256, True), (15, 4, 257, True), (15, 4, 1000, True), (15, 4, 1024, True), (15, 4, 100_000, True),
    (15, 4, 100_001, True), (15, 4, 500_000, True),
    (15, 4, 1024, False),       # full workgroups only on the direct path: a multiple of 256 is always a whole number of float4, so by a misaligned view
]

# points_rgb_groups: (Pk, Pe, edit levels); keep levels 4, 16 coefficients in both groups; edit positions [Pe,3] and [Pe,1]
GROUP_CASES = [(1000, 2052, 4), (1001, 2051, 1), (257, 100_000, 3)]

# direction mode with directions that are not unit vectors (the kernels must not normalise them): (entry point, M, levels, P)
NON_UNIT_CASES = [("rgb", 16, 4, 1001), ("dcrest", 16, 4, 1000)]


def _seed(*key):
    """one seed per input set.  The leading constant is the first of 20261, 1, 2, ... with which the CPU tests below hold for every case: with a
    few hundred rows "at most 1e-4 of the rows undecidable" means none (a 1000-row case has one with probability ~1e-2), and at P = 1 the
    whole-tensor bar is a bar on one row that cancellation can push any fp32 evaluation over -- conditions on the inputs and the reference,
    decided by test_fp32_restatement_is_within_the_row_bars without the kernels."""
    return int((1 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))


def make_inputs(P, M, levels, unit=True, pos_cols=3):
    """seeded: sh ~ 0.6 N(0,1), positions N(0,1), the camera at CAM, upstream N(0,1), unit directions (or of lengths in [0.5, 2])"""
    rng = np.random.default_rng(_seed(P, M, levels, unit, pos_cols))
    d = rng.standard_normal((P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if not unit:
        d *= rng.uniform(0.5, 2.0, (P, 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"sh": t(0.6 * rng.standard_normal((P, M, 3))), "pos": t(rng.standard_normal((P, pos_cols))), "cam": t(np.asarray(CAM)),
            "up": t(rng.standard_normal((P, 3))), "dirs": t(d)}


def _mode_kw(inp, mode):
    return {"positions": inp["pos"], "camera_centers": inp["cam"]} if mode == "camera" else {"directions": inp["dirs"]}


def judge(inp, levels, mode, got):
    """-> the distances of ``got`` from the float64 reference on the device of the inputs: whole tensors (rel_l2) and rows (units of u)"""
    f64 = lambda t: t.detach().to(torch.float64)
    kw = _mode_kw(inp, mode)
    want = R.reference(inp["sh"], levels, inp["up"], **kw)
    scales = R.row_scales(f64(inp["sh"]), levels, f64(inp["up"]), **{k: f64(v) for k, v in kw.items()})
    rep = R.row_distances(got, want, scales, levels)
    keep = (~scales["undecidable"]).cpu().numpy()
    n = lambda t: f64(t).cpu().numpy()
    rep["colors"] = util.rel_l2(n(got["colors"]), n(want["colors"]))
    if got.get("dsh") is not None:
        rep["dsh"] = util.rel_l2(n(got["dsh"])[keep], n(want["dsh"])[keep])
        if levels > 1:
            rep["dvec"] = util.rel_l2(n(got["dvec"])[keep], n(want["dvec"])[keep])
    return rep


def check(rep, P, name=None):
    print(name, {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in rep.items()})
    if name is not None:
        util.record_parity(name, rep)
    for k, tol in WHOLE_TOL.items():
        assert rep.get(k, 0.0) <= tol, (k, rep[k])
    assert rep["colors_u"] <= R.COLOR_U
    assert rep.get("dsh_u", 0.0) <= R.DSH_U
    assert rep.get("dvec_u", 0.0) <= R.DDIR_U
    assert rep.get("dsh_nonzero_above_levels", 0) == 0 and rep.get("dsh_nonzero_clamped_rows", 0) == 0
    assert rep.get("dvec_nonzero_at_one_level", 0) == 0
    assert rep["excluded_rows"] <= MAX_EXCLUDED_SHARE * P, rep["excluded_rows"]


# ------------------------------------------------------------------------------------------------------------------------------ CPU

def test_dcrest_cases_cover_every_path():
    """the case table reaches the three data paths of k_sh_rgb_dcrest with one workgroup, full workgroups only and a ragged last workgroup, the
    untouched rest tensor (one level) too, and holds the benchmark's shapes"""
    cells = {R.dcrest_path(P, Mr, l, a) for Mr, l, P, a in DCREST_CASES}
    assert {(p, b) for p in ("staged", "lds_out", "direct") for b in ("one", "full", "ragged")} <= cells
    assert any(p is None for p, _ in cells)
    assert {(15, 4, 500_000, True), (15, 1, 500_000, True)} <= set(DCREST_CASES)
    assert {Mr for Mr, *_ in DCREST_CASES} == {0, 3, 5, 8, 14, 15}
    assert {(Mr, l) for Mr, l, *_ in DCREST_CASES} == {(Mr, l) for Mr in (0, 3, 5, 8, 14, 15) for l in _valid_levels(Mr + 1)}
    # the rule itself at the shapes the kernel's comments name
    assert R.dcrest_path(500_000, 15, 4) == ("staged", "ragged") and R.dcrest_path(301, 15, 4) == ("direct", "ragged")
    assert R.dcrest_path(200, 15, 2) == ("lds_out", "one") and R.dcrest_path(1024, 15, 4, aligned=False) == ("direct", "full")
    assert R.dcrest_path(1024, 15, 1) == (None, "full") and R.dcrest_path(256, 8, 3) == ("staged", "one")


def _reference_cases():
    """every distinct input set of the matrix: (P, M, levels, unit directions, position columns)"""
    cases = {(P, M, l, True, 3) for M, l, P in RGB_CASES} | {(P, Mr + 1, l, True, 3) for Mr, l, P, _ in DCREST_CASES}
    cases |= {(P, M, l, False, 3) for _, M, l, P in NON_UNIT_CASES}
    cases |= {(Pe, 16, l, True, c) for _, Pe, l in GROUP_CASES for c in (3, 1)} | {(Pk, 16, 4, True, 3) for Pk, _, _ in GROUP_CASES}
    return sorted(cases)


@pytest.mark.parametrize("P,M,levels,unit,pos_cols", _reference_cases())
def test_fp32_restatement_is_within_the_row_bars(P, M, levels, unit, pos_cols):
    """the bars are reachable without the code under test: the restatement itself in fp32 (CPU, autograd) stays within every row bar of its
    float64 evaluation, and at most 1e-4 of the rows are undecidable -- for the inputs of every case of the matrix"""
    inp = make_inputs(P, M, levels, unit, pos_cols)
    for mode in (("camera", "direction") if unit and pos_cols == 3 else ("camera",) if unit else ("direction",)):
        got = R.reference(inp["sh"], levels, inp["up"], dtype=torch.float32, **_mode_kw(inp, mode))
        check(judge(inp, levels, mode, got), P)


# ------------------------------------------------------------------------------------------------------------------------------ GPU

def _leaf(t, dev, misaligned=False):
    """a leaf on the device; misaligned: a contiguous view one float into its buffer (4-byte but not 16-byte aligned)"""
    t = t.to(dev)
    if misaligned:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        t = v
    return t.detach().requires_grad_()


def run_rgb(inp, levels, mode, dev, mis=()):
    from youreditableavatar_amd import sh_color
    sh = _leaf(inp["sh"], dev, "sh" in mis)
    vec = _leaf(inp["pos"] if mode == "camera" else inp["dirs"], dev, "vec" in mis)
    kw = {"positions": vec, "camera_centers": inp["cam"].to(dev)} if mode == "camera" else {"directions": vec}
    col = sh_color.points_rgb(sh, levels, **kw)
    col.backward(_upstream(inp["up"], dev, mis))
    return {"colors": col.detach(), "dsh": sh.grad, "dvec": vec.grad}


def _upstream(up, dev, mis):
    if "up" in mis:
        return _leaf(up, dev, True).detach()
    if "up_strided" in mis:
        wide = torch.zeros(up.shape[0], 4, device=dev)
        wide[:, :3] = up.to(dev)
        return wide[:, :3]
    return up.to(dev)


def run_dcrest(inp, levels, mode, dev, mis=()):
    """-> the result with "dsh" = cat(dc gradient, rest gradient); at one level the rest tensor is handed over full of NaN (it must not be
    read) and must get no gradient"""
    from youreditableavatar_amd import sh_color
    M = inp["sh"].shape[1]
    dc = _leaf(inp["sh"][:, :1].contiguous(), dev, "dc" in mis)
    rest = None
    if M > 1:
        rest = _leaf(torch.full_like(inp["sh"][:, 1:], float("nan")) if levels == 1 else inp["sh"][:, 1:].contiguous(), dev, "rest" in mis)
    vec = _leaf(inp["pos"] if mode == "camera" else inp["dirs"], dev, "vec" in mis)
    kw = {"positions": vec, "camera_centers": inp["cam"].to(dev)} if mode == "camera" else {"directions": vec}
    col = sh_color.points_rgb_dc_rest(dc, rest, levels, **kw)
    col.backward(_upstream(inp["up"], dev, mis))
    if levels == 1:
        assert rest is None or rest.grad is None
        d_rest = torch.zeros(dc.shape[0], M - 1, 3, device=dev)
    else:
        d_rest = rest.grad
    return {"colors": col.detach(), "dsh": torch.cat([dc.grad, d_rest], dim=1), "dvec": vec.grad}


def _same_bits(a, b, keys=("colors", "dsh", "dvec")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _on(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("M,levels,P", RGB_CASES)
def test_points_rgb_rows(M, levels, P, gpu_device):
    """k_sh_rgb: the staged path (M == 16) and the row-wise one, every (M, levels), P across the workgroup boundaries; two runs give the same bits"""
    inp = make_inputs(P, M, levels)
    for mode in ("camera", "direction"):
        got = run_rgb(inp, levels, mode, gpu_device)
        check(judge(_on(inp, gpu_device), levels, mode, got), P, f"sh_rows_rgb_M{M}_L{levels}_P{P}_{mode}")
        assert _same_bits(got, run_rgb(inp, levels, mode, gpu_device)), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("Mr,levels,P,aligned", DCREST_CASES)
def test_points_rgb_dc_rest_rows(Mr, levels, P, aligned, gpu_device):
    """k_sh_rgb_dcrest on the path dcrest_path names; the same bits as points_rgb on the concatenation (colours and SH gradients) and from
    two runs"""
    inp = make_inputs(P, Mr + 1, levels)
    path, blocks = R.dcrest_path(P, Mr, levels, aligned)
    mis = () if aligned else ("rest",)
    for mode in ("camera", "direction"):
        got = run_dcrest(inp, levels, mode, gpu_device, mis)
        check(judge(_on(inp, gpu_device), levels, mode, got), P, f"sh_rows_dcrest_Mr{Mr}_L{levels}_P{P}_{path}_{blocks}{'' if aligned else '_misaligned'}_{mode}")
        assert _same_bits(got, run_dcrest(inp, levels, mode, gpu_device, mis)), "two runs differ"
        assert _same_bits(got, run_rgb(inp, levels, mode, gpu_device), ("colors", "dsh")), "points_rgb on the concatenation differs"


@pytest.mark.gpu
@pytest.mark.parametrize("entry,M,levels,P", NON_UNIT_CASES)
def test_directions_are_not_normalised(entry, M, levels, P, gpu_device):
    inp = make_inputs(P, M, levels, unit=False)
    got = (run_rgb if entry == "rgb" else run_dcrest)(inp, levels, "direction", gpu_device)
    check(judge(_on(inp, gpu_device), levels, "direction", got), P, f"sh_rows_{entry}_nonunit_M{M}_L{levels}_P{P}")


@pytest.mark.gpu
@pytest.mark.parametrize("pos_cols", [3, 1])
@pytest.mark.parametrize("Pk,Pe,elev", GROUP_CASES)
def test_points_rgb_groups_rows(Pk, Pe, elev, pos_cols, gpu_device):
    """points_rgb_groups: two launches of k_sh_rgb_dcrest into one colour tensor, the second at a 12 Pk-byte offset of the colours and of the
    upstream gradient (odd Pk: 4-byte aligned only).  Colours of both groups and the edit group's gradients row by row; the keep group gets none."""
    from youreditableavatar_amd import sh_color
    dev = gpu_device
    keep, edit = make_inputs(Pk, 16, 4), make_inputs(Pe, 16, elev, pos_cols=pos_cols)
    g = lambda t, grad=True: t.contiguous().to(dev).requires_grad_(grad)
    kdc, krest, kpos = g(keep["sh"][:, :1], False), g(keep["sh"][:, 1:], False), g(keep["pos"], False)
    runs = []
    for _ in range(2):
        edc, erest, epos = g(edit["sh"][:, :1]), g(edit["sh"][:, 1:]), g(edit["pos"])
        col = sh_color.points_rgb_groups(keep_sh_dc=kdc, keep_sh_rest=krest, keep_sh_levels=4, keep_positions=kpos, edit_sh_dc=edc, edit_sh_rest=erest,
                                         edit_sh_levels=elev, edit_positions=epos, camera_centers=edit["cam"].to(dev))
        col.backward(torch.cat([keep["up"], edit["up"]]).to(dev))
        if elev == 1:
            assert erest.grad is None
        d_rest = erest.grad if elev > 1 else torch.zeros_like(erest)
        runs.append({"colors": col.detach(), "dsh": torch.cat([edc.grad, d_rest], dim=1), "dvec": epos.grad})
    assert _same_bits(*runs)
    assert kdc.grad is None and krest.grad is None and kpos.grad is None
    assert runs[0]["dvec"].shape == (Pe, pos_cols)
    tag = f"sh_rows_groups_Pk{Pk}_Pe{Pe}_L{elev}_pos{pos_cols}"
    check(judge(_on(keep, dev), 4, "camera", {"colors": runs[0]["colors"][:Pk]}), Pk, tag + "_keep")
    check(judge(_on(edit, dev), elev, "camera", {**runs[0], "colors": runs[0]["colors"][Pk:]}), Pe, tag + "_edit")


def _edge_inputs(levels):
    """64 ordinary rows, then: row 0 exactly at the camera centre (the max(|v|, 1e-12) branch of the normalisation: a finite gradient of order
    1e12); rows 1-8 with all three channels clamped; row 9 (meaningful at one level) with dc[0] such that the fp32 product with the kernel's
    SH_C0 is exactly -0.5 -- see the module docstring"""
    inp = make_inputs(64, 16, levels)
    inp["pos"][0] = inp["cam"]
    inp["sh"][1:9] *= 0.01
    inp["sh"][1:9, 0] = -5.0
    c0 = np.float32(R.C0)
    dc = np.float32(-0.5) / c0
    cands = [dc]
    for _ in range(4):
        cands = [np.nextafter(cands[0], np.float32(-4)), *cands, np.nextafter(cands[-1], np.float32(0))]
    exact = [x for x in cands if np.float32(c0 * x) == np.float32(-0.5)]
    assert exact, "no fp32 dc whose product with SH_C0 rounds to -0.5"
    inp["sh"][9, 0, 0] = float(exact[0])
    return inp


def _check_edges(rep, levels, got):
    """the edge case's own undecidable row (9, at one level) replaces the share condition"""
    assert rep.pop("excluded_rows") == (1 if levels == 1 else 0)
    check({**rep, "excluded_rows": 0}, 64)
    assert bool(torch.isfinite(got["dvec"]).all())
    if levels > 1:
        assert float(got["dvec"][0].abs().max()) > 1e9           # row 0: divided by max(|v|, 1e-12), not by |v| = 0
    assert bool((got["colors"][1:9] == 0).all()) and bool((got["dsh"][1:9] == 0).all()) and bool((got["dvec"][1:9] == 0).all())


@pytest.mark.parametrize("levels", [1, 2, 4])
def test_edge_rows_fp32_restatement(levels):
    inp = _edge_inputs(levels)
    got = R.reference(inp["sh"], levels, inp["up"], dtype=torch.float32, **_mode_kw(inp, "camera"))
    _check_edges(judge(inp, levels, "camera", got), levels, got)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 4])
@pytest.mark.parametrize("entry", ["rgb", "dcrest"])
def test_edge_rows(entry, levels, gpu_device):
    inp = _edge_inputs(levels)
    got = (run_rgb if entry == "rgb" else run_dcrest)(inp, levels, "camera", gpu_device)
    _check_edges(judge(_on(inp, gpu_device), levels, "camera", got), levels, got)


def _framed(dev, shape, front=64):
    """a NaN-filled tensor in the middle of a larger buffer of canaries (16-byte aligned: 64 floats in) -> (buffer, the tensor, front)"""
    n = int(np.prod(shape))
    big = torch.full((front + n + 64,), CANARY, device=dev)
    big[front:front + n] = float("nan")
    return big, big[front:front + n].view(shape), front


def _framed_ok(frame):
    big, inner, front = frame
    n = inner.numel()
    return (not bool(torch.isnan(inner).any())) and bool((big[:front] == CANARY).all()) and bool((big[front + n:] == CANARY).all())


# (entry point, rest rows (M - 1), levels, P, data path of the dc / rest kernel)
STORE_CASES = [("dcrest", 15, 4, 1000, "staged"), ("dcrest", 15, 2, 1000, "lds_out"), ("dcrest", 15, 4, 1001, "direct"), ("rgb", 15, 4, 1001, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["camera", "direction"])
@pytest.mark.parametrize("entry,Mr,levels,P,path", STORE_CASES)
def test_stores_stay_inside_their_tensors(entry, Mr, levels, P, path, mode, gpu_device):
    """through the C ABI, the ragged last workgroup of each path: every output is a NaN-filled slice in the middle of a buffer of canaries.
    Afterwards no NaN is left inside (every element written, the zeros above the active levels too), every canary in front and behind is
    intact, and the values are those of the autograd entry point bit for bit."""
    from youreditableavatar_amd import sh_color
    dev = gpu_device
    if path is not None:
        assert R.dcrest_path(P, Mr, levels) == (path, "ragged")
    inp = _on(make_inputs(P, Mr + 1, levels), dev)
    want = (run_rgb if entry == "rgb" else run_dcrest)(inp, levels, mode, dev)
    cam = mode == "camera"
    vec = (inp["pos"] if cam else inp["dirs"]).contiguous()
    p = lambda t: None if t is None else t.data_ptr()
    pos, cc, dirs = (p(vec), p(inp["cam"]), None) if cam else (None, None, p(vec))
    st = torch.cuda.current_stream(dev).cuda_stream
    f_col, f_vec = _framed(dev, (P, 3)), _framed(dev, (P, 3))
    if entry == "rgb":
        sh = inp["sh"].contiguous()
        f_sh = _framed(dev, (P, Mr + 1, 3))
        r = sh_color._lib.tgs_sh_rgb_forward(st, P, Mr + 1, levels, p(sh), pos, cc, dirs, p(f_col[1]))
        assert r >= 0
        r = sh_color._lib.tgs_sh_rgb_backward(st, P, Mr + 1, levels, p(sh), pos, cc, dirs, p(inp["up"]), p(f_sh[1]), p(f_vec[1]) if cam else None,
                                              None if cam else p(f_vec[1]))
        assert r >= 0
        frames, dsh = (f_col, f_vec, f_sh), f_sh[1]
    else:
        dc, rest = inp["sh"][:, :1].contiguous(), inp["sh"][:, 1:].contiguous()
        f_dc, f_rest = _framed(dev, (P, 1, 3)), _framed(dev, (P, Mr, 3))
        r = sh_color._lib.tgs_sh_rgb_dcrest_forward(st, P, Mr, levels, p(dc), p(rest), pos, cc, dirs, p(f_col[1]))
        assert r >= 0
        r = sh_color._lib.tgs_sh_rgb_dcrest_backward(st, P, Mr, levels, p(dc), p(rest), pos, cc, dirs, p(inp["up"]), p(f_dc[1]), p(f_rest[1]),
                                                     p(f_vec[1]) if cam else None, None if cam else p(f_vec[1]))
        assert r >= 0
        frames, dsh = (f_col, f_vec, f_dc, f_rest), torch.cat([f_dc[1], f_rest[1]], dim=1)
    torch.cuda.synchronize(dev)
    assert all(_framed_ok(f) for f in frames), [_framed_ok(f) for f in frames]
    assert torch.equal(f_col[1], want["colors"]) and torch.equal(dsh, want["dsh"]) and torch.equal(f_vec[1], want["dvec"])
    assert bool((dsh[:, levels * levels:] == 0).all())


ALIGNMENT_CASES = [("rgb", 16, 4, 1001, m) for m in (("sh",), ("vec",), ("up",), ("up_strided",))] + \
                  [("rgb", 16, 2, 100_000, ("sh",))] + \
                  [("dcrest", 16, 4, 1000, m) for m in (("rest",), ("dc",), ("vec",), ("up",), ("up_strided",))] + \
                  [("dcrest", 16, 2, 1000, ("rest",)), ("dcrest", 9, 3, 100_000, ("rest",))]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["camera", "direction"])
@pytest.mark.parametrize("entry,M,levels,P,mis", ALIGNMENT_CASES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_misaligned_views_give_the_same_bits(entry, M, levels, P, mis, mode, gpu_device):
    """one tensor at a time 4-byte but not 16-byte aligned (a contiguous view one float into its buffer), or the upstream gradient not
    contiguous: the float4 paths are left for the scalar ones and the result is that of the aligned call bit for bit, multi-workgroup P"""
    run = run_rgb if entry == "rgb" else run_dcrest
    inp = make_inputs(P, M, levels)
    assert _same_bits(run(inp, levels, mode, gpu_device, mis), run(inp, levels, mode, gpu_device))


@pytest.mark.gpu
def test_rest_slice_of_a_wider_parameter(gpu_device):
    """rest[:, :8] of a 15-row parameter (not contiguous: copied on the way in) at three levels: the staged path on the copy, the gradient back
    on the parameter with zeros in the rows that were cut off"""
    from youreditableavatar_amd import sh_color
    P, dev = 1001, gpu_device
    inp = make_inputs(P, 16, 3)
    dc, rest, pos = _leaf(inp["sh"][:, :1].contiguous(), dev), _leaf(inp["sh"][:, 1:].contiguous(), dev), _leaf(inp["pos"], dev)
    col = sh_color.points_rgb_dc_rest(dc, rest[:, :8], 3, positions=pos, camera_centers=inp["cam"].to(dev))
    col.backward(inp["up"].to(dev))
    want = run_dcrest({**inp, "sh": inp["sh"][:, :9].contiguous()}, 3, "camera", dev)
    assert torch.equal(col.detach(), want["colors"]) and torch.equal(torch.cat([dc.grad, rest.grad[:, :8]], dim=1), want["dsh"])
    assert torch.equal(pos.grad, want["dvec"]) and bool((rest.grad[:, 8:] == 0).all())
