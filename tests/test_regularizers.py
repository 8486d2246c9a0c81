"""youreditableavatar_amd.regularizers (csrc/tgs_reg.hip): the per-Gaussian circumradii and the scaling regulariser of the refinement loops
(Edit_core/tetgs_texture/refine.py:306-317, refine_3dgs.py:339-350), against tests/golden/ref_scale_reg_fixture.npz -- what the reference's
OWN ``TetGS.radii`` / ``Edit3DTetGS.radii`` return and what the loop's arithmetic gives in float64 on the classes' own ``scaling`` /
``edit_scaling`` (tests/make_ref_scale_reg_fixture.py) -- and against that arithmetic restated in torch (``loop_term``) on the CPU.

THE BARS.  Which rows are selected: IDENTICAL to torch's CPU float32 evaluation of the same float32 inputs -- no row left out, none tolerated.
Radii: every finite one within 3e-7 relative of the float64 value rounded to float32, non-finite exactly where the reference's are.  The
value: <= 3e-7 relative to the float64 mean over the selected set.  Gradients: rel-L2 <= 3e-6 (the two bars of tests/test_bind.py), exactly 0
on every entry that is not a selected row's first maximum.  Everything else is bit for bit.  Figures are printed before they are asserted."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import util
from tests.test_abi import HEADER, declared_functions, lib_path

FIX = os.path.join(util.GOLDEN_DIR, "ref_scale_reg_fixture.npz")
CASES = ("tetgs.one", "tetgs.three", "edit3d")
ENTRY_POINTS = ("tgs_gaussian_radii", "tgs_scale_reg_workspace_bytes", "tgs_scale_reg_forward", "tgs_scale_reg_backward")
TOL_OUT, TOL_GRAD = 3e-7, 3e-6


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def loop_term(scaling, radii, max_factor=1.0, ratio_threshold=10.0):
    """refine.py:308-317 (refine_3dgs.py:341-350 on edit_scaling) with its two constants as arguments -> (term, a zero that carries no
    gradient when the loop adds nothing; the boolean row mask)"""
    big = scaling.max(dim=-1).values
    small = scaling.min(dim=-1).values
    mask = (big > radii * max_factor) & (big / small > ratio_threshold)
    return (big[mask].mean() if mask.sum() > 0 else scaling.sum() * 0), mask


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_and_the_library_exports_them():
    fns = declared_functions()
    text = open(HEADER).read()
    lib = ctypes.CDLL(lib_path())
    for f in ENTRY_POINTS:
        assert f in fns, f
        assert hasattr(lib, f), f"libtgs_raster.so does not export {f}"
    for cite in ("refine.py:306-317", "refine_3dgs.py:339-350", "tetgs_model.py:299-310", "tetgs_edit_3d.py:332-343", "graphics_utils.py:109-116"):
        assert cite in text, cite
    assert int(re.search(r"#define TGS_ABI_VERSION (\d+)", text).group(1)) == 3
    from youreditableavatar_amd import build
    assert "tgs_reg.hip" in build.SOURCES


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = ctypes.CDLL(lib_path())
    vp, it, fl, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    lib.tgs_last_error.restype = ctypes.c_char_p
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    X, INVALID = 4096, -1
    lib.tgs_scale_reg_workspace_bytes.restype, lib.tgs_scale_reg_workspace_bytes.argtypes = sz, [it]
    wb = lib.tgs_scale_reg_workspace_bytes
    assert (wb(-1), wb(0), wb(1), wb(256), wb(257), wb(500_000)) == (0, 0, 16, 16, 32, 16 * 1954)
    lib.tgs_scale_reg_forward.restype, lib.tgs_scale_reg_forward.argtypes = it, [vp, it, vp, it, vp, fl, fl, vp, vp, vp, sz]
    fwd = dict(stream=None, P=1000, scales=X, raw=0, radii=X, max_factor=1.0, ratio_threshold=10.0, codes=X, out3=X, workspace=X, workspace_bytes=64)
    call = lambda fn, base, **over: fn(*{**base, **over}.values())
    assert call(lib.tgs_scale_reg_forward, fwd, P=-1) == INVALID and msg() == "tgs_scale_reg_forward: P < 0"
    for p in ("scales", "radii", "codes", "out3", "workspace"):
        for raw in (0, 1):
            assert call(lib.tgs_scale_reg_forward, fwd, raw=raw, **{p: None}) == INVALID and msg() == "tgs_scale_reg_forward: NULL required pointer", p
    assert call(lib.tgs_scale_reg_forward, fwd, P=0, out3=None) == INVALID and "NULL" in msg()
    assert call(lib.tgs_scale_reg_forward, fwd, workspace_bytes=63) == INVALID and "tgs_scale_reg_forward: workspace smaller" in msg()
    assert call(lib.tgs_scale_reg_forward, fwd, P=1025, workspace_bytes=64) == INVALID and "workspace" in msg()
    lib.tgs_scale_reg_backward.restype, lib.tgs_scale_reg_backward.argtypes = it, [vp, it, vp, vp, vp, vp, fl, it, vp]
    bwd = dict(stream=None, P=1000, codes=X, out3=X, raw_scales=None, upstream=None, weight=1.0, accumulate=0, grad=X)
    assert call(lib.tgs_scale_reg_backward, bwd, P=-3) == INVALID and msg() == "tgs_scale_reg_backward: P < 0"
    for p in ("codes", "out3", "grad"):
        for acc in (0, 1):
            assert call(lib.tgs_scale_reg_backward, bwd, accumulate=acc, **{p: None}) == INVALID and msg() == "tgs_scale_reg_backward: NULL required pointer", p
    assert call(lib.tgs_scale_reg_backward, bwd, P=0, codes=None, out3=None, grad=None) == 0           # nothing to do, nothing launched
    lib.tgs_gaussian_radii.restype, lib.tgs_gaussian_radii.argtypes = it, [vp, it, it, it, vp, vp, it, vp, it, vp, vp]
    rad = dict(stream=None, V=10, F=5, P=7, verts=X, faces=X, faces_i64=0, face_indices=X, index_kind=0, radii=X, invalid_flag=X)
    for k in ("V", "F", "P"):
        assert call(lib.tgs_gaussian_radii, rad, **{k: -1}) == INVALID and msg() == "tgs_gaussian_radii: bad sizes", k
    for kind in (-1, 3):
        assert call(lib.tgs_gaussian_radii, rad, index_kind=kind) == INVALID and "tgs_gaussian_radii: index_kind" in msg()
    for k in ("V", "F"):                                   # Gaussians bound to an empty mesh: every index is out of range, known from the sizes
        assert call(lib.tgs_gaussian_radii, rad, **{k: 0}) == INVALID and "tgs_gaussian_radii" in msg() and "out of range" in msg(), k
    for p in ("verts", "faces", "face_indices", "radii", "invalid_flag"):
        assert call(lib.tgs_gaussian_radii, rad, **{p: None}) == INVALID and msg() == "tgs_gaussian_radii: NULL required pointer", p
    assert call(lib.tgs_gaussian_radii, rad, P=0, verts=None, faces=None, face_indices=None, radii=None, invalid_flag=None) == 0


def test_regularizers_refuse_cpu_tensors_loudly():
    from youreditableavatar_amd import regularizers as R
    s, r = torch.rand(5, 3), torch.rand(5)
    for fn in (R.scaling_regularizer, R.scaling_regularizer_raw, R.scaling_reg_value_and_grad):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(s, r)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.gaussian_radii(torch.rand(4, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))


def _np_radii(verts, faces, idx):
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = lambda d: np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    a, b, c = n(B - C), n(A - C), n(A - B)
    s = (a + b + c) / 2
    with np.errstate(all="ignore"):
        R = a * b * c / (4 * np.sqrt(s * (s - a) * (s - b) * (s - c)))
    return R[idx.reshape(-1).astype(np.int64)]             # (.astype truncates the float indices like .int())


def _np_term(scaling, radii, mf, rt):
    """-> value, mask, gradient with respect to scaling: 1 / count on the FIRST maximum of every selected row"""
    big, small = scaling.max(axis=1), scaling.min(axis=1)
    with np.errstate(all="ignore"):
        mask = (big > radii * mf) & (big / small > rt)
    g = np.zeros_like(scaling)
    if mask.sum():
        g[np.nonzero(mask)[0], scaling.argmax(axis=1)[mask]] = 1.0 / mask.sum()
    return (big[mask].mean() if mask.sum() else 0.0), mask, g


def test_fixture_is_self_consistent(fx):
    """numpy float64 from the stored inputs reproduces the stored radii, values, masks and gradients to 1e-12; the fixture holds what it is
    meant to hold (degenerate faces, float indices, [P,1] indices, ties, margins)."""
    for case in CASES:
        verts, faces, idx, radii = fx[f"{case}.verts"], fx[f"{case}.faces"], fx[f"{case}.face_indices"], fx[f"{case}.radii"]
        assert verts.dtype == np.float64 and np.array_equal(verts, verts.astype(np.float32).astype(np.float64))
        mine = _np_radii(verts, faces, idx)
        fin = np.isfinite(radii)
        assert np.array_equal(np.isfinite(mine), fin) and np.array_equal(np.isnan(mine), np.isnan(radii))
        assert np.isnan(radii).sum() >= 4 and np.isposinf(radii).sum() >= 3 and fin.sum() > 0.9 * len(radii)
        assert np.abs(mine[fin] / radii[fin] - 1).max() <= 1e-12
        raw, scaling = fx[f"{case}.raw_scales"], fx[f"{case}.scaling"]
        assert np.array_equal(raw, raw.astype(np.float32).astype(np.float64))
        assert np.abs(np.exp(raw) / scaling - 1).max() <= 1e-12
        ties2 = (scaling[:, 1] == scaling[:, 2]) & (scaling[:, 0] < scaling[:, 1])
        ties3 = (scaling[:, 0] == scaling[:, 1]) & (scaling[:, 1] == scaling[:, 2])
        assert ties2.sum() >= 40 and ties3.sum() >= 40
        for k in (0, 1):
            mf, rt = fx[f"{case}.set{k}.settings"]
            value, mask, g = _np_term(scaling, radii, mf, rt)
            assert np.array_equal(mask, fx[f"{case}.set{k}.mask"]) and 0 < mask.sum() < len(mask)
            assert abs(value / float(fx[f"{case}.set{k}.value"]) - 1) <= 1e-12
            assert np.abs(g - fx[f"{case}.set{k}.grad_scaling"]).max() <= 1e-12 * np.abs(g).max()
            assert np.abs(g * scaling - fx[f"{case}.set{k}.grad_raw"]).max() <= 1e-12 * np.abs(g * scaling).max()
            assert (mask & ties2).sum() >= 5, "selected two-way ties pin autograd's choice: the lowest index"
            big = scaling.max(axis=1)
            with np.errstate(all="ignore"):
                assert np.abs(big[fin] / (radii[fin] * mf) - 1).min() >= 1e-4 and np.abs(big / scaling.min(axis=1) / rt - 1).min() >= 1e-4
        assert (fx[f"{case}.set1.mask"] & ties3).sum() >= 5        # (ratio 1: only the second setting lets a three-way tie through)
    assert fx["edit3d.face_indices"].dtype == np.float32                    # Edit3DTetGS keeps float indices (tetgs_model.py:719)
    assert fx["tetgs.three.face_indices"].shape == (900, 1) and fx["tetgs.one.face_indices"].dtype == np.int64


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------

def _dev(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def _rel(x, ref):
    return abs(float(x) - float(ref)) / abs(float(ref)) if float(ref) != 0 else abs(float(x))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_gaussian_radii_against_the_reference_classes(fx, case, gpu_device):
    from youreditableavatar_amd.regularizers import gaussian_radii
    verts, faces, idx, want = fx[f"{case}.verts"], fx[f"{case}.faces"], fx[f"{case}.face_indices"], fx[f"{case}.radii"]
    want32 = want.astype(np.float32)
    fin = np.isfinite(want)
    v = _dev(verts, gpu_device)
    for fdt in (torch.int64, torch.int32):
        for idt in (torch.int32, torch.int64, torch.float32, torch.float64, torch.int16):
            got = gaussian_radii(v, _dev(faces, gpu_device, fdt), _dev(idx, gpu_device, idt)).cpu().numpy()
            assert got.shape == (want.shape[0],) and got.dtype == np.float32
            err = np.abs(got[fin].astype(np.float64) / want32[fin].astype(np.float64) - 1).max()
            print(f"{case} faces {fdt} indices {idt}: finite radii max rel err {err:.3e}; non-finite {int((~fin).sum())}")
            assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want))
            assert np.array_equal(np.isposinf(got), np.isposinf(want))
            assert err <= TOL_OUT
    # float indices are truncated as .int() truncates them
    frac = _dev(idx.reshape(-1).astype(np.float64) + 0.75, gpu_device, torch.float32)
    assert np.array_equal(gaussian_radii(v, _dev(faces, gpu_device, torch.int64), frac).cpu().numpy(), got, equal_nan=True)
    assert gaussian_radii(v, _dev(faces, gpu_device, torch.int64), torch.zeros(0, dtype=torch.int64, device=gpu_device)).shape == (0,)


@pytest.mark.gpu
def test_gpu_gaussian_radii_rejects_indices_out_of_range(gpu_device):
    from youreditableavatar_amd.regularizers import gaussian_radii
    v = torch.rand(10, 3, device=gpu_device)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]], device=gpu_device)
    ok = gaussian_radii(v, f, torch.tensor([0, 1, 1], device=gpu_device))
    assert torch.isfinite(ok).all()
    for bad in (torch.tensor([0, 2]), torch.tensor([-1, 0]), torch.tensor([0.0, 2.0]), torch.tensor([float("nan"), 0.0]), torch.tensor([0.0, -1.0]),
                torch.tensor([0, 1 << 40])):
        with pytest.raises(RuntimeError, match="TGS_ERR_INVALID"):
            gaussian_radii(v, f, bad.to(gpu_device))
    for badf in ([[0, 1, 10], [3, 4, 5]], [[0, -1, 2], [3, 4, 5]]):
        with pytest.raises(RuntimeError, match="TGS_ERR_INVALID"):
            gaussian_radii(v, torch.tensor(badf, device=gpu_device), torch.tensor([0, 1], device=gpu_device))
    assert float(gaussian_radii(v, f, torch.tensor([-0.5, 1.9], device=gpu_device))[1]) == float(ok[1])      # .int() truncates toward zero
    with pytest.raises(RuntimeError, match="out of range"):
        gaussian_radii(v, torch.zeros(0, 3, dtype=torch.int64, device=gpu_device), torch.tensor([0], device=gpu_device))


def _special_rows():
    """float32 rows on and next to both thresholds -> (scaling [N,3], radii [N])"""
    f = np.float32
    up, dn = lambda x: np.nextafter(f(x), f(np.inf)), lambda x: np.nextafter(f(x), f(-np.inf))
    rows, radii = [], []

    def add(s, r):
        rows.append([f(x) for x in s]); radii.append(f(r))

    for r in (0.3, 1.0, 0.0123456, 7.5):
        for big in (f(r), up(r), dn(r)):                                       # max == radius exactly, one unit above, one below
            add((1e-8, big, big * f(0.5)), r); add((big, 1e-8, 1e-8), r); add((1e-8, 1e-8, big), r)
    for small in (0.5, 0.1, 0.3, 1.7e-3, 3.3333333):                           # a ratio of exactly 10 where it is representable, and one unit round it
        for big in (f(small) * f(10), up(f(small) * f(10)), dn(f(small) * f(10))):
            for sm in (f(small), up(small), dn(small)):
                add((sm, big, sm), 1e-6); add((big, sm, big), 1e-6)
    rng = np.random.default_rng(5)
    for small in rng.uniform(1e-3, 2.0, 400).astype(f):                        # fp32(10 * small) / small is 10 or one unit off: the division's rounding decides
        big = f(small * f(10))
        add((small, big, small * f(2)), 1e-6); add((small, up(big), small), 1e-6); add((small, dn(big), small * f(3)), 1e-6)
    for r in (0.1, 1.0):
        add((0.0, 1.0, 2.0), r); add((0.0, 0.0, 2.0), r); add((0.0, 0.0, 0.0), r); add((2.0, 0.0, 2.0), r)          # min == 0: inf > 10; 0 / 0: not selected
    for r in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        add((1e-8, 1.0, 2.0), r); add((3.0, 3.0, 1e-8), r)
    add((1e-8, np.inf, 1.0), 1.0); add((np.nan, 5.0, 1e-8), 1.0); add((1e-8, 5.0, np.nan), 1.0); add((np.inf, np.inf, 1e-8), np.inf)
    for x in (0.7, 2.5):                                                       # ties of the maximum, two- and three-way, in every position
        add((x, x, 1e-8), 0.1); add((x, 1e-8, x), 0.1); add((1e-8, x, x), 0.1); add((x, x, x), 0.1)
        add((x, x, x * 0.01), 0.1); add((x * 0.01, x, x), 0.1)
    return np.array(rows, f), np.array(radii, f)


def _check_activated(scaling32, radii32, mf, rt, dev, label):
    """the selected set against torch's CPU float32 evaluation; value and gradient against float64 over that set"""
    from youreditableavatar_amd.regularizers import scaling_regularizer
    s_cpu, r_cpu = torch.tensor(scaling32), torch.tensor(radii32)
    _, mask = loop_term(s_cpu, r_cpu, mf, rt)
    mask = mask.numpy()
    s = torch.tensor(scaling32, device=dev, requires_grad=True)
    value, codes = scaling_regularizer(s, torch.tensor(radii32, device=dev), mf, rt, return_codes=True)
    value.backward()
    codes, grad = codes.cpu().numpy(), s.grad.cpu().numpy()
    assert codes.dtype == np.uint8 and codes.shape == mask.shape
    assert np.array_equal(codes != 0, mask), (label, "selected set differs from torch's float32 evaluation", np.nonzero((codes != 0) != mask)[0][:10])
    s64 = scaling32.astype(np.float64)
    finite_rows = ~np.isnan(s64).any(axis=1)
    first = np.where(finite_rows, np.argmax(np.where(np.isnan(s64), -np.inf, s64), axis=1), 0)
    assert np.array_equal(codes[mask], first[mask] + 1), (label, "argmax: the lowest index among equal maxima")
    want_g = np.zeros_like(s64)
    if mask.sum():
        want_g[np.nonzero(mask)[0], first[mask]] = 1.0 / mask.sum()
    assert np.array_equal(grad != 0, want_g != 0), (label, "gradient entries that must be exactly 0")
    big = s64.max(axis=1)[mask]
    want_v = big.mean() if mask.sum() else 0.0
    print(f"{label}: {int(mask.sum())} of {len(mask)} rows selected; value {float(value):.9g} vs {want_v:.9g} rel {_rel(value, want_v) if np.isfinite(want_v) else float('nan'):.3e}; "
          f"grad rel-L2 {util.rel_l2(grad, want_g):.3e}")
    if np.isfinite(want_v):
        assert _rel(value, want_v) <= TOL_OUT
    else:
        assert not np.isfinite(float(value))
    assert util.rel_l2(grad, want_g) <= TOL_GRAD
    return mask, codes


@pytest.mark.gpu
def test_gpu_activated_form_selects_exactly_what_torch_selects(fx, gpu_device):
    scaling, radii = _special_rows()
    keep = np.isfinite(scaling).all(axis=1)                                    # (an infinite maximum makes the mean infinite: checked on its own below)
    mask, _ = _check_activated(scaling[keep], radii[keep], 1.0, 10.0, gpu_device, "special rows")
    assert 100 < mask.sum() < len(mask) - 100
    _check_activated(scaling[keep], radii[keep], 0.5, 0.5, gpu_device, "special rows, (0.5, 0.5)")
    _check_activated(scaling, radii, 1.0, 10.0, gpu_device, "special rows with inf / NaN scales")
    # the rows the thresholds are about, one by one (radius 1e-6 or 0.1: the first condition holds)
    one = lambda s, r: int(_check_activated(np.array([s], np.float32), np.array([r], np.float32), 1.0, 10.0, gpu_device, f"row {s} radius {r}")[1][0])
    assert one((1e-8, 1.0, 0.5), 1.0) == 0 and one((1e-8, np.nextafter(np.float32(1), np.float32(2)), 0.5), 1.0) == 2        # max == radius is not >
    assert one((0.5, 5.0, 0.5), 1e-6) == 0 and one((0.5, np.nextafter(np.float32(5), np.float32(6)), 0.5), 1e-6) == 2       # a ratio of exactly 10 is not >
    assert one((0.0, 1.0, 2.0), 0.1) == 3 and one((0.0, 0.0, 0.0), 0.1) == 0
    assert one((1e-8, 1.0, 2.0), np.nan) == 0 and one((1e-8, 1.0, 2.0), np.inf) == 0 and one((1e-8, 1.0, 2.0), -np.inf) == 3
    assert one((2.5, 2.5, 1e-8), 0.1) == 1 and one((1e-8, 2.5, 2.5), 0.1) == 2 and one((2.5, 1e-8, 2.5), 0.1) == 1
    for case in CASES:
        for k in (0, 1):
            mf, rt = (float(x) for x in fx[f"{case}.set{k}.settings"])
            _check_activated(fx[f"{case}.scaling"].astype(np.float32), fx[f"{case}.radii"].astype(np.float32), mf, rt, gpu_device, f"{case} set{k}")
    scaling, radii = _special_rows()
    rng = np.random.default_rng(11)
    _check_activated(scaling[rng.permutation(len(scaling))[:129]], radii[:129], 1.0, 10.0, gpu_device, "shuffled")


def _hold_to_fixture(label, value, grad, want_value, want_grad):
    print(f"{label}: value {float(value):.9g} vs {float(want_value):.9g} rel {_rel(value, want_value):.3e}; grad rel-L2 {util.rel_l2(grad, want_grad):.3e}")
    assert _rel(value, want_value) <= TOL_OUT
    assert util.rel_l2(grad, want_grad) <= TOL_GRAD
    assert np.array_equal(np.asarray(grad) != 0, want_grad != 0), (label, "the gradient's pattern: selected rows' first maximum only")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_both_forms_against_the_reference_arithmetic(fx, case, gpu_device):
    """activated form on the classes' scaling, raw form on their raw scales, radii from gaussian_radii: value and gradient of the fixture
    (float64 autograd of the loop's arithmetic), ties on the lowest index as the fixture pins them"""
    from youreditableavatar_amd.regularizers import gaussian_radii, scaling_reg_value_and_grad, scaling_regularizer, scaling_regularizer_raw
    radii = gaussian_radii(_dev(fx[f"{case}.verts"], gpu_device), _dev(fx[f"{case}.faces"], gpu_device, torch.int64),
                           _dev(fx[f"{case}.face_indices"], gpu_device, torch.float32 if case == "edit3d" else torch.int64))
    raw64 = fx[f"{case}.raw_scales"]
    r64 = fx[f"{case}.radii"]
    for k in (0, 1):
        mf, rt = (float(x) for x in fx[f"{case}.set{k}.settings"])
        # no row within 1e-5 relative of either threshold, in float64 from the float32 inputs: one unit of a device expf cannot flip a decision
        e = np.exp(raw64.astype(np.float32).astype(np.float64))
        big, small, fin = e.max(axis=1), e.min(axis=1), np.isfinite(r64)
        assert np.abs(big[fin] / (r64[fin] * mf) - 1).min() >= 1e-5 and np.abs(big / small / rt - 1).min() >= 1e-5
        want_v, want_mask = float(fx[f"{case}.set{k}.value"]), fx[f"{case}.set{k}.mask"]
        s = _dev(fx[f"{case}.scaling"], gpu_device).requires_grad_(True)
        v, codes = scaling_regularizer(s, radii, mf, rt, return_codes=True)
        v.backward()
        assert np.array_equal(codes.cpu().numpy() != 0, want_mask)
        _hold_to_fixture(f"{case} set{k} activated", v, s.grad.cpu().numpy(), want_v, fx[f"{case}.set{k}.grad_scaling"])
        raw = _dev(raw64, gpu_device).requires_grad_(True)
        v, codes = scaling_regularizer_raw(raw, radii, mf, rt, return_codes=True)
        (v * 1.0).backward()
        assert np.array_equal(codes.cpu().numpy() != 0, want_mask)
        _hold_to_fixture(f"{case} set{k} raw", v, raw.grad.cpu().numpy(), want_v, fx[f"{case}.set{k}.grad_raw"])
        v2, g2 = scaling_reg_value_and_grad(raw.detach(), radii, mf, rt)
        assert torch.equal(v2, v.detach()) and torch.equal(g2, raw.grad)                       # the form without autograd: the same kernels


def _cloud_inputs(P, dev, seed=2, flat=None):
    """raw scales of a synthetic cloud with the flat axis of mesh-bound Gaussians (log(1e-8), tetgs_edit_2d.py:203; or `flat` times the row's
    largest scale) on every other row, and radii around the largest scale"""
    from youreditableavatar_amd import scenes
    cloud = scenes.make_cloud(P, 0, seed=seed, scale_mult=2.0)
    rng = np.random.default_rng(seed)
    raw = np.log(np.asarray(cloud["scales"], np.float32))
    raw[::2, rng.integers(0, 3)] = np.log(1e-8) if flat is None else (raw.max(axis=1) + np.log(flat))[::2]
    radii = (np.exp(raw).max(axis=1) * np.exp(rng.uniform(-0.7, 0.7, P))).astype(np.float32)
    return torch.tensor(raw, device=dev), torch.tensor(radii, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 5000, 500_000])
def test_gpu_raw_form_is_the_activated_form_on_the_bound_scaling(P, gpu_device):
    """sizes; raw == activated on gaussian_bind's scaling bit for bit (the same expf); two calls give the same bits; weight, upstream and
    accumulate; against the loop's arithmetic in torch on the CPU"""
    from youreditableavatar_amd.bindings import gaussian_bind
    from youreditableavatar_amd.regularizers import scaling_reg_value_and_grad, scaling_regularizer, scaling_regularizer_raw
    raw0, radii = _cloud_inputs(P, gpu_device)
    if P == 1:
        raw0 = torch.log(torch.tensor([[1e-8, 0.5, 0.25]], device=gpu_device)); radii = torch.tensor([0.3], device=gpu_device)
    raw_a, raw_b = raw0.clone().requires_grad_(True), raw0.clone().requires_grad_(True)
    _, scaling, _, _ = gaussian_bind(raw_scales=raw_a)
    va, ca = scaling_regularizer(scaling, radii, return_codes=True)
    vb, cb = scaling_regularizer_raw(raw_b, radii, return_codes=True)
    va.backward(); vb.backward()
    assert torch.equal(ca, cb) and int((ca != 0).sum()) > 0
    assert torch.equal(va, vb) and torch.equal(raw_a.grad, raw_b.grad)
    # the loop's lines in float32 on the CPU select the same rows (same float32 scaling); float64 gives value and gradient
    s_cpu = scaling.detach().cpu()
    _, mask = loop_term(s_cpu, radii.cpu())
    assert np.array_equal(mask.numpy(), ca.cpu().numpy() != 0)
    s64 = s_cpu.double().requires_grad_(True)
    t64, _ = loop_term(s64, radii.cpu().double())
    t64.backward()
    print(f"P={P}: {int(mask.sum())} rows selected, {-(-P // 256)} partials; value rel {_rel(va, t64):.3e}; raw grad rel-L2 {util.rel_l2(raw_a.grad.cpu().numpy(), (s64.grad * s64).detach().numpy()):.3e}")
    assert _rel(va, t64) <= TOL_OUT
    assert util.rel_l2(raw_a.grad.cpu().numpy(), (s64.grad * s64).detach().numpy()) <= TOL_GRAD
    # reproducibility
    v1, g1 = scaling_reg_value_and_grad(raw0, radii)
    v2, g2 = scaling_reg_value_and_grad(raw0, radii)
    assert torch.equal(v1, v2) and torch.equal(g1, g2) and torch.equal(v1, vb.detach()) and torch.equal(g1, raw_b.grad)
    # weight: the gradient of weight * value, bit for bit the scaled gradient for a power of two; the value stays the unweighted term
    vw, gw = scaling_reg_value_and_grad(raw0, radii, weight=0.125)
    assert torch.equal(vw, v1) and torch.equal(gw, g1 * 0.125)
    # upstream through autograd
    raw_c = raw0.clone().requires_grad_(True)
    (scaling_regularizer_raw(raw_c, radii) * 0.125).backward()
    assert torch.equal(raw_c.grad, gw)
    raw_d = raw0.clone().requires_grad_(True)
    (scaling_regularizer_raw(raw_d, radii) * 3.0).backward()
    assert util.rel_l2(raw_d.grad.cpu().numpy(), 3.0 * g1.double().cpu().numpy()) <= 1e-7
    # accumulate: prior + gradient, to one unit in the last place per element; a poisoned buffer is overwritten without it
    prior = torch.randn(P, 3, device=gpu_device) * float(g1.abs().max())
    buf = prior.clone()
    v3, out = scaling_reg_value_and_grad(raw0, radii, grad_out=buf, accumulate=True, weight=0.125)
    assert out is buf and torch.equal(v3, v1)
    want = prior.double() + gw.double()
    ulp = torch.tensor(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32)), dtype=torch.float64, device=gpu_device)
    assert bool(((buf.double() - want).abs() <= ulp).all())
    assert torch.equal(buf[ca == 0], prior[ca == 0])
    poisoned = torch.full((P, 3), float("nan"), device=gpu_device)
    scaling_reg_value_and_grad(raw0, radii, grad_out=poisoned)
    assert torch.equal(poisoned, g1)
    with pytest.raises(RuntimeError, match="accumulate=True needs"):
        scaling_reg_value_and_grad(raw0, radii, accumulate=True)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 300, 100_000])
def test_gpu_no_row_selected_gives_zero_and_a_zero_gradient(P, gpu_device):
    from youreditableavatar_amd.regularizers import scaling_reg_value_and_grad, scaling_regularizer, scaling_regularizer_raw
    raw, _ = _cloud_inputs(P, gpu_device)
    radii = torch.full((P,), 1e6, device=gpu_device)                           # every splat well inside its face's circumcircle
    for fn, x in ((scaling_regularizer, torch.exp(raw)), (scaling_regularizer_raw, raw)):
        x = x.clone().requires_grad_(True)
        v, codes = fn(x, radii, return_codes=True)
        (v * 2.0).backward()
        assert v.dim() == 0 and float(v) == 0.0 and not torch.signbit(v) and int(codes.sum()) == 0
        assert x.grad.shape == (P, 3) and int(torch.count_nonzero(x.grad)) == 0
    poisoned = torch.full((P, 3), float("nan"), device=gpu_device)
    v, g = scaling_reg_value_and_grad(raw, radii, grad_out=poisoned)
    assert float(v) == 0.0 and g is poisoned and int(torch.count_nonzero(poisoned)) == 0 and not torch.isnan(poisoned).any()
    prior = torch.randn(P, 3, device=gpu_device)
    buf = prior.clone()
    scaling_reg_value_and_grad(raw, radii, grad_out=buf, accumulate=True)
    assert torch.equal(buf, prior)
    # and with no Gaussians at all
    e = torch.zeros(0, 3, device=gpu_device, requires_grad=True)
    v = scaling_regularizer_raw(e, torch.zeros(0, device=gpu_device))
    v.backward()
    assert float(v) == 0.0 and e.grad.shape == (0, 3)


@pytest.mark.gpu
def test_gpu_row_slice_of_a_grouped_bind(gpu_device):
    """refine_3dgs.py:343-344 reads edit_scaling: the edit rows of the two-group bind's scaling; the gradient reaches _edit_scales only"""
    from youreditableavatar_amd.bindings import gaussian_bind_groups
    from youreditableavatar_amd.regularizers import scaling_regularizer, scaling_regularizer_raw
    Pk, Pe = 1001, 777                                                         # (the slice starts 12 012 bytes in: 4-byte aligned only)
    rng = np.random.default_rng(4)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu_device)
    keep_raw, _ = _cloud_inputs(Pk, gpu_device, seed=8)
    edit_raw, radii = _cloud_inputs(Pe, gpu_device, seed=9)
    edit_raw.requires_grad_(True)
    kw = dict(keep_points=t(rng.standard_normal((Pk, 3))), keep_densities=t(rng.standard_normal((Pk, 1))), keep_scales=keep_raw, keep_quaternions=t(rng.standard_normal((Pk, 4))),
              edit_densities=t(rng.standard_normal((Pe, 1))).requires_grad_(True), edit_scales=edit_raw, edit_quaternions=t(rng.standard_normal((Pe, 4))).requires_grad_(True),
              edit_points=t(rng.standard_normal((Pe, 3))).requires_grad_(True))
    _, scaling, _, _ = gaussian_bind_groups(**kw)
    v, codes = scaling_regularizer(scaling[Pk:], radii, return_codes=True)
    v.backward()
    ref = edit_raw.detach().clone().requires_grad_(True)
    vr, cr = scaling_regularizer_raw(ref, radii, return_codes=True)
    vr.backward()
    assert int((codes != 0).sum()) > 50 and torch.equal(codes, cr) and torch.equal(v, vr)
    assert torch.equal(edit_raw.grad, ref.grad) and keep_raw.grad is None
    assert int(torch.count_nonzero(kw["edit_densities"].grad)) == 0 and int(torch.count_nonzero(kw["edit_quaternions"].grad)) == 0


@pytest.mark.gpu
def test_gpu_three_training_steps_with_the_regulariser(gpu_device):
    """bind -> rasterizer -> l1_ssim_loss + scaling_regularizer -> FusedAdam, three steps on a small scene.  The rasterizer's gradient at
    `scaling` is recorded at every step (its sums are float atomics: two loops that each render cannot be held to a bar of roundings) and the
    steps are replayed on the CPU with the loop's lines in torch -- exp, the lines, autograd, torch.optim.Adam(foreach=False) -- in float64
    (truth) and float32 (yardstick).  The bar of tests/test_optim.py: the kernel path's rel-L2 error on the displacement of `_scales` and on
    Adam's two moments, and its max-abs error on `_scales`, each <= 2 x the float32 torch run's own distance from float64."""
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.bindings import gaussian_bind
    from youreditableavatar_amd.loss import l1_ssim_loss
    from youreditableavatar_amd.optim import FusedAdam
    from youreditableavatar_amd.regularizers import scaling_regularizer
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = gpu_device
    P, W, H = 3000, 160, 128
    cloud = scenes.make_cloud(P, 0, seed=21, scale_mult=3.0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    op = np.clip(cloud["opacities"], 1e-4, 1 - 1e-4)
    raw0, radii = _cloud_inputs(P, dev, seed=21, flat=0.02)                    # (a flat axis of 1e-8 puts its gradients below the bar's 1e-18: see tests/test_optim.py)
    L = {"points": t(cloud["means3D"]), "all_densities": t(np.log(op / (1 - op))), "scales": raw0.clone(), "quaternions": t(cloud["rotations"])}
    for p in L.values():
        p.requires_grad_(True)
    # colours and target from a generator of the test's own (the cloud's seed): drawn from torch's global state they were whatever the tests
    # before this one left, and for some states (2 of 40 tried) a gradient of the flat axis lands in (0, 1e-18), outside the bar's condition below
    gen = torch.Generator(device=dev).manual_seed(21)
    colors = torch.rand(P, 3, device=dev, generator=gen)
    lrs = {"points": 1.6e-4, "all_densities": 0.05, "scales": 0.005, "quaternions": 0.001}
    opt = FusedAdam([{"params": [p], "lr": lrs[n], "name": n} for n, p in L.items()], lr=0.0, eps=1e-15)
    cams = [scenes.orbit_camera(W, H, azimuth_deg=a) for a in (10.0, 130.0, 250.0)]
    gt = torch.rand(3, H, W, device=dev, generator=gen)
    recorded, selected, raw_grads = [], [], []
    for c in cams:
        rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
                                           projmatrix=t(c.projmatrix), sh_degree=0, campos=t(c.campos), prefiltered=False, debug=False)
        for p in L.values():
            p.grad = None
        opacity, scaling, quats, _ = gaussian_bind(L["all_densities"], L["scales"], L["quaternions"])
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        to_raster = scaling.view_as(scaling)                                   # an alias whose gradient is the rasterizer's share alone, as this loop saw it
        to_raster.register_hook(lambda g: recorded.append(g.detach().cpu().numpy()))
        img, _ = GaussianRasterizer(rs)(means3D=L["points"], means2D=m2, opacities=opacity, colors_precomp=colors, scales=to_raster, rotations=quats)
        photometric = l1_ssim_loss(img, gt, 0.2)
        reg, codes = scaling_regularizer(scaling, radii, return_codes=True)
        selected.append(int((codes != 0).sum()))
        (photometric + reg).backward()
        raw_grads.append(L["scales"].grad.cpu().numpy())
        opt.step()
    assert len(recorded) == 3 and min(selected) > 100 and float(np.abs(recorded[0]).max()) > 0
    for g in raw_grads:                                                        # the bar's condition on its inputs (tests/test_optim.py): |g| is 0 or >= 1e-18
        assert ((g == 0) | (np.abs(g) >= 1e-18)).all()
    st = opt.state[L["scales"]]
    f = lambda x: x.detach().double().cpu().numpy()
    ours = (f(L["scales"]), f(st["exp_avg"]), f(st["exp_avg_sq"]))
    init = raw0.cpu().numpy()

    def replay(dtype):
        p = torch.nn.Parameter(torch.tensor(init, dtype=dtype))
        o = torch.optim.Adam([p], lr=lrs["scales"], eps=1e-15, foreach=False)
        r = radii.cpu().to(dtype)
        for g in recorded:
            p.grad = None
            s = torch.exp(p)
            term, _ = loop_term(s, r)
            ((s * torch.tensor(g, dtype=dtype)).sum() + term).backward()
            o.step()
        return f(p), f(o.state[p]["exp_avg"]), f(o.state[p]["exp_avg_sq"])

    yard, truth = replay(torch.float32), replay(torch.float64)
    p0 = init.astype(np.float64)
    figures = [(n, util.rel_l2(ours[k], truth[k]), util.rel_l2(yard[k], truth[k])) for n, k in (("exp_avg", 1), ("exp_avg_sq", 2))]
    figures.append(("displacement", util.rel_l2(ours[0] - p0, truth[0] - p0), util.rel_l2(yard[0] - p0, truth[0] - p0)))
    figures.append(("param max-abs", float(np.abs(ours[0] - truth[0]).max()), float(np.abs(yard[0] - truth[0]).max())))
    failures = []
    for what, mine, ref in figures:
        print(f"three steps, rows selected {selected}: {what:14s} kernel path {mine:.3e}  fp32 torch {ref:.3e}  ratio {mine / ref if ref > 0 else float('nan'):.3f}")
        assert np.isfinite(mine)
        if mine > 2.0 * ref:
            failures.append((what, mine, ref))
    assert not failures, failures
