"""The rest of the reference's utils/loss_utils.py: l2_loss, ssim(size_average=False), the per-image and pointwise forms for the batch path.
Pinned to the reference's own outputs (tests/golden/ref_loss_ext_fixture.npz, written by tests/make_ref_loss_ext_fixture.py) and to the
float64 evaluation of oracle/loss_ref.py.  Tolerances are those of tests/test_loss.py: fixture rtol 2e-6 / gradient rel-L2 1e-5, float64
rtol 1e-5 / 1e-5 -- an order of magnitude above the reference's own fp32 distance from float64 (the fixture records it per case:
<= 1.5e-7 for values, <= 1.5e-6 for gradients)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import loss_ref
from tests import util

FX = os.path.join(util.GOLDEN_DIR, "ref_loss_ext_fixture.npz")
SSIM_CASES = "abcd"             # [B,C,H,W] = (2,3,37,53), (4,1,9,70), (1,3,16,16), (3,3,64,96)
L2_CASES = "abcdefg"            # + [C,H,W] = (1,1,1), (3,7,11), (3,16,16)


def ref_l2(p, g):
    """loss_utils.py:20-21 restated"""
    return ((p - g) ** 2).mean()


def ref_ssim_per_image(p, g):
    """loss_utils.py:60-63 with size_average=False restated: one mean per image of the [B,C,H,W] map"""
    return loss_ref.ssim_map(p, g).mean((-3, -2, -1))


def _case(fx, name, dtype=torch.float32):
    return torch.tensor(fx[f"{name}_pred"], dtype=dtype, requires_grad=True), torch.tensor(fx[f"{name}_gt"], dtype=dtype)


def test_fixture_holds_every_case():
    fx = np.load(FX)
    assert "".join(fx["cases_ssim"]) == SSIM_CASES and "".join(fx["cases_l2"]) == L2_CASES
    shapes = {n: fx[f"{n}_pred"].shape for n in L2_CASES}
    assert [shapes[n] for n in SSIM_CASES] == [(2, 3, 37, 53), (4, 1, 9, 70), (1, 3, 16, 16), (3, 3, 64, 96)]
    assert shapes["e"] == (1, 1, 1) and fx["f_pred"].size % 4 != 0
    assert all((fx[f"{n}_pred"] == fx[f"{n}_gt"]).any() for n in SSIM_CASES)          # pixels with pred == gt exactly
    assert all(len(set(fx[f"{n}_w"].tolist())) == fx[f"{n}_w"].size for n in "abd")    # non-uniform upstream weights
    assert all(fx[f"{n}_fp64_distance"][1::2].max() <= 1e-5 for n in L2_CASES)
    assert str(fx["ssim_3d_per_image_error"]) == "IndexError"


@pytest.mark.parametrize("name", L2_CASES)
def test_restatement_reproduces_reference(name):
    """what the GPU tests evaluate in float64, evaluated in fp32, is the reference's recorded output"""
    fx = np.load(FX)
    p, g = _case(fx, name)
    v = ref_l2(p, g)
    (dv,) = torch.autograd.grad(v, p)
    np.testing.assert_allclose(v.detach().numpy(), fx[f"{name}_l2"], rtol=1e-6)
    assert util.rel_l2(dv.numpy(), fx[f"{name}_dl2"]) <= 1e-6
    if name in SSIM_CASES:
        s = ref_ssim_per_image(p, g)
        (ds,) = torch.autograd.grad((s * torch.tensor(fx[f"{name}_w"])).sum(), p)
        np.testing.assert_allclose(s.detach().numpy(), fx[f"{name}_ssim"], rtol=1e-6)
        assert util.rel_l2(ds.numpy(), fx[f"{name}_dssim"]) <= 1e-6


def test_trainer_import_line_works():
    """`from utils.loss_utils import ssim, l1_loss, l2_loss` (refine.py:11, refine_3dgs.py:14, paint_2dgs.py:15) with the package swapped in"""
    from youreditableavatar_amd import loss
    names = [str(n) for n in np.load(FX)["trainer_imports"]]
    assert set(names) >= {"ssim", "l1_loss", "l2_loss"}
    for n in names:
        assert callable(getattr(loss, n, None)), f"youreditableavatar_amd.loss has no {n}"
    ns = {}
    exec("from youreditableavatar_amd.loss import " + ", ".join(names), ns)


def test_cpu_tensors_are_refused():
    from youreditableavatar_amd import loss
    z = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError):
        loss.l2_loss(z, z)
    with pytest.raises(RuntimeError):
        loss.pixel_value_and_grad(z, z, "l1")
    with pytest.raises(RuntimeError):
        loss.ssim(z[None], z[None], size_average=False)
    with pytest.raises(ValueError):
        loss.pixel_value_and_grad(z, z, "huber")


def test_new_entry_points_validate_without_a_gpu():
    from youreditableavatar_amd import build
    lib = ctypes.CDLL(build.build_native())
    vp, it, i64, fl, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    lib.tgs_last_error.restype = ctypes.c_char_p
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    INVALID, X = -1, 4096                       # X: a fake non-NULL pointer (nothing is dereferenced before the checks)
    lib.tgs_pixel_loss_workspace_bytes.restype, lib.tgs_pixel_loss_workspace_bytes.argtypes = sz, [it, i64]
    lib.tgs_l1_ssim_images_workspace_bytes.restype, lib.tgs_l1_ssim_images_workspace_bytes.argtypes = sz, [it, it, it, it]
    lib.tgs_l1_ssim_workspace_bytes.restype, lib.tgs_l1_ssim_workspace_bytes.argtypes = sz, [it, it, it]
    assert lib.tgs_pixel_loss_workspace_bytes(0, 100) == 0 and lib.tgs_pixel_loss_workspace_bytes(2, 0) == 0 and lib.tgs_pixel_loss_workspace_bytes(-1, -5) == 0
    assert 0 < lib.tgs_pixel_loss_workspace_bytes(8, 3 * 1080 * 1920) <= 1 << 20
    assert lib.tgs_l1_ssim_images_workspace_bytes(0, 3, 8, 8) == 0 and lib.tgs_l1_ssim_images_workspace_bytes(2, 0, 8, 8) == 0
    assert lib.tgs_l1_ssim_images_workspace_bytes(2, 3, 0, 8) == 0 and lib.tgs_l1_ssim_images_workspace_bytes(2, 3, 8, -1) == 0
    assert lib.tgs_l1_ssim_images_workspace_bytes(4, 3, 108, 192) == lib.tgs_l1_ssim_workspace_bytes(12, 108, 192) > 0
    big = 1 << 30

    lib.tgs_pixel_loss.restype, lib.tgs_pixel_loss.argtypes = it, [vp, it, it, i64, vp, vp, vp, vp, vp, sz]
    good = dict(kind=1, images=2, n=100, img=X, gt=X, out=X, grad=None, ws=X, nbytes=big)
    for over in (dict(kind=2), dict(kind=-1), dict(images=0), dict(n=0), dict(n=-4), dict(img=None), dict(gt=None), dict(out=None), dict(ws=None), dict(images=65536),
                 dict(nbytes=16)):
        assert lib.tgs_pixel_loss(None, *{**good, **over}.values()) == INVALID and "tgs_pixel_loss:" in msg(), over
    assert "workspace" in msg()

    lib.tgs_pixel_loss_backward.restype, lib.tgs_pixel_loss_backward.argtypes = it, [vp, it, it, i64, vp, vp, vp, it, vp]
    good = dict(kind=0, images=2, n=100, img=X, gt=X, upstream=None, per_image=0, grad=X)
    for over in (dict(kind=7), dict(images=0), dict(n=0), dict(img=None), dict(gt=None), dict(grad=None), dict(images=70000)):
        assert lib.tgs_pixel_loss_backward(None, *{**good, **over}.values()) == INVALID and "tgs_pixel_loss_backward:" in msg(), over

    lib.tgs_l1_ssim_images.restype, lib.tgs_l1_ssim_images.argtypes = it, [vp, it, it, it, it, vp, vp, fl, vp, vp, vp, sz]
    good = dict(images=2, channels=3, h=8, w=8, img=X, gt=X, f=0.2, out=X, grad=None, ws=X, nbytes=big)
    for over in (dict(images=0), dict(channels=0), dict(h=0), dict(w=-1), dict(img=None), dict(gt=None), dict(out=None), dict(ws=None), dict(nbytes=100),
                 dict(images=300, channels=300), dict(h=64 * 65536)):
        assert lib.tgs_l1_ssim_images(None, *{**good, **over}.values()) == INVALID and "tgs_l1_ssim_images:" in msg(), over

    lib.tgs_l1_ssim_images_backward.restype, lib.tgs_l1_ssim_images_backward.argtypes = it, [vp, it, it, it, it, vp, vp, fl, vp, it, vp, vp, sz]
    good = dict(images=2, channels=3, h=8, w=8, img=X, gt=X, f=0.2, upstream=None, per_image=1, grad=X, ws=X, nbytes=big)
    for over in (dict(images=-1), dict(channels=0), dict(h=0), dict(w=0), dict(img=None), dict(gt=None), dict(grad=None), dict(ws=None), dict(nbytes=100),
                 dict(images=65536, channels=1)):
        assert lib.tgs_l1_ssim_images_backward(None, *{**good, **over}.values()) == INVALID and "tgs_l1_ssim_images_backward:" in msg(), over
    # the entry points that were there keep their own names in their messages
    lib.tgs_l1_ssim.restype, lib.tgs_l1_ssim.argtypes = it, [vp, it, it, it, vp, vp, fl, vp, vp, vp, sz]
    assert lib.tgs_l1_ssim(None, 3, 8, 8, X, X, 0.2, X, None, X, 100) == INVALID and msg() == "tgs_l1_ssim: workspace smaller than tgs_l1_ssim_workspace_bytes()"
    lib.tgs_l1_ssim_backward.restype, lib.tgs_l1_ssim_backward.argtypes = it, [vp, it, it, it, vp, vp, fl, vp, vp, vp, sz]
    assert lib.tgs_l1_ssim_backward(None, 3, 8, 0, X, X, 0.2, None, X, X, big) == INVALID and msg().startswith("tgs_l1_ssim_backward: positive sizes")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _inputs(shape, seed=None):
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    gt = rng.uniform(0, 1, shape).astype(np.float32)
    return np.clip(gt + rng.normal(0, 0.1, shape), 0, 1).astype(np.float32), gt


def _report(label, got, want, grad_dist):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    print(f"{label}: value rel {np.max(np.abs(got - want) / np.abs(want)):.3g}, gradient rel-L2 {grad_dist:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", L2_CASES)
def test_gpu_l2_matches_reference_fixture(name):
    from youreditableavatar_amd import loss
    fx = np.load(FX)
    p, g = torch.tensor(fx[f"{name}_pred"]).cuda().requires_grad_(True), torch.tensor(fx[f"{name}_gt"]).cuda()
    v = loss.l2_loss(p, g)
    v.backward()
    d = util.rel_l2(p.grad.cpu().numpy(), fx[f"{name}_dl2"])
    _report(f"l2 {name}", v.item(), fx[f"{name}_l2"], d)
    assert v.dim() == 0 and p.grad.shape == p.shape
    np.testing.assert_allclose(v.item(), fx[f"{name}_l2"], rtol=2e-6)
    assert d <= 1e-5
    assert torch.all(p.grad[p == g] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SSIM_CASES)
def test_gpu_ssim_per_image_matches_reference_fixture(name):
    from youreditableavatar_amd import loss
    fx = np.load(FX)
    p, g = torch.tensor(fx[f"{name}_pred"]).cuda().requires_grad_(True), torch.tensor(fx[f"{name}_gt"]).cuda()
    s = loss.ssim(p, g, size_average=False)
    assert tuple(s.shape) == (p.shape[0],)
    (s * torch.tensor(fx[f"{name}_w"]).cuda()).sum().backward()
    d = util.rel_l2(p.grad.cpu().numpy(), fx[f"{name}_dssim"])
    _report(f"ssim per image {name}", s.detach().cpu().numpy(), fx[f"{name}_ssim"], d)
    np.testing.assert_allclose(s.detach().cpu().numpy(), fx[f"{name}_ssim"], rtol=2e-6)
    assert d <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 5, 200), (1, 33, 17), (2, 3, 40, 56), (3, 1080, 1920), (4, 3, 1080, 1920),
                                   (3, 7, 1003)])      # 7021 elements per image: not a multiple of 4 and several 1024-element steps (per_image: the 4-byte path over several workgroups)
def test_gpu_l2_matches_fp64(shape):
    from youreditableavatar_amd import loss
    pred, gt = _inputs(shape)
    p64 = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    want = ref_l2(p64, torch.tensor(gt, dtype=torch.float64))
    (dwant,) = torch.autograd.grad(want, p64)
    p = torch.tensor(pred).cuda().requires_grad_(True)
    got = loss.l2_loss(p, torch.tensor(gt).cuda())
    (3.0 * got).backward()                                      # the incoming gradient as a device scalar
    d = util.rel_l2(p.grad.cpu().numpy() / 3.0, dwant.numpy())
    _report(f"l2 {shape}", got.item(), want.item(), d)
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-5)
    assert d <= 1e-5
    # the sync-free forms, whole tensor and per image, both kinds
    for kind, fn in (("l2", lambda a, b: (a - b) ** 2), ("l1", lambda a, b: (a - b).abs())):
        e64 = fn(p64.detach(), torch.tensor(gt, dtype=torch.float64))
        q = p64.detach().clone().requires_grad_(True)
        (dall,) = torch.autograd.grad(fn(q, torch.tensor(gt, dtype=torch.float64)).sum(), q)
        v, gr = loss.pixel_value_and_grad(p.detach(), torch.tensor(gt).cuda(), kind)
        np.testing.assert_allclose(v.item(), e64.mean().item(), rtol=1e-5)
        assert util.rel_l2(gr.cpu().numpy(), (dall / e64.numel()).numpy()) <= 1e-5, kind
        vb, gb = loss.pixel_value_and_grad(p.detach(), torch.tensor(gt).cuda(), kind, per_image=True)
        per = e64[0].numel()
        np.testing.assert_allclose(vb.cpu().numpy(), e64.reshape(shape[0], -1).mean(1).numpy(), rtol=1e-5)
        assert util.rel_l2(gb.cpu().numpy(), (dall / per).numpy()) <= 1e-5, kind


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 40, 56), (1, 1, 33, 17), (4, 3, 1080, 1920)])
def test_gpu_ssim_per_image_matches_fp64(shape):
    from youreditableavatar_amd import loss
    pred, gt = _inputs(shape)
    w = np.random.default_rng(1).uniform(0.25, 2.0, shape[0])
    want, dwant = [], []
    for b in range(shape[0]):                                   # image by image: the float64 graph of the whole batch is several GB at 1080p
        p64 = torch.tensor(pred[b:b + 1], dtype=torch.float64, requires_grad=True)
        s64 = ref_ssim_per_image(p64, torch.tensor(gt[b:b + 1], dtype=torch.float64))
        (d64,) = torch.autograd.grad(w[b] * s64.sum(), p64)
        want.append(s64.item()); dwant.append(d64.numpy())
    p = torch.tensor(pred).cuda().requires_grad_(True)
    got = loss.ssim(p, torch.tensor(gt).cuda(), size_average=False)
    (3.0 * (got * torch.tensor(w, dtype=torch.float32).cuda()).sum()).backward()
    d = util.rel_l2(p.grad.cpu().numpy() / 3.0, np.concatenate(dwant))
    _report(f"ssim per image {shape}", got.detach().cpu().numpy(), want, d)
    np.testing.assert_allclose(got.detach().cpu().numpy(), np.array(want), rtol=1e-5)
    assert d <= 1e-5


@pytest.mark.gpu
def test_gpu_l2_takes_a_misaligned_view():
    """a view whose storage offset leaves data_ptr 4-byte but not 16-byte aligned goes through the 4-byte path"""
    from youreditableavatar_amd import loss
    pred, gt = _inputs((3, 50, 70), seed=9)
    n = pred.size
    want = ref_l2(torch.tensor(pred, dtype=torch.float64), torch.tensor(gt, dtype=torch.float64)).item()
    dwant = 2.0 * (pred.astype(np.float64) - gt) / n
    for off_p, off_g in ((1, 0), (0, 3), (2, 2)):
        sp, sg = torch.zeros(n + 8).cuda(), torch.zeros(n + 8).cuda()
        p = sp[off_p:off_p + n].view(3, 50, 70)
        g = sg[off_g:off_g + n].view(3, 50, 70)
        p.copy_(torch.tensor(pred)); g.copy_(torch.tensor(gt))
        assert p.is_contiguous() and (p.data_ptr() % 16 != 0 or g.data_ptr() % 16 != 0) and p.data_ptr() % 4 == 0
        p = p.detach().requires_grad_(True)
        v = loss.l2_loss(p, g)
        v.backward()
        np.testing.assert_allclose(v.item(), want, rtol=1e-5)
        assert util.rel_l2(p.grad.cpu().numpy(), dwant) <= 1e-5
        assert torch.all(sp[:off_p] == 0) and torch.all(sp[off_p + n:] == 0)


@pytest.mark.gpu
def test_gpu_per_image_is_each_image_alone():
    from youreditableavatar_amd import loss
    pred, gt = _inputs((3, 3, 75, 120), seed=4)
    p, g = torch.tensor(pred).cuda(), torch.tensor(gt).cuda()
    out, grad = loss.l1_ssim_value_and_grad(p, g, 0.2, per_image=True)
    assert tuple(out.shape) == (3, 3) and grad.shape == p.shape
    for b in range(3):
        o1, g1 = loss.l1_ssim_value_and_grad(p[b], g[b], 0.2)
        np.testing.assert_allclose(out[b].cpu().numpy(), o1.cpu().numpy(), rtol=2e-6)
        assert util.rel_l2(grad[b].cpu().numpy(), g1.cpu().numpy()) <= 1e-6
    # a batch of one and a [C,H,W] image are the whole-tensor call
    o0, g0 = loss.l1_ssim_value_and_grad(p[1], g[1], 0.2)
    for a, b in ((p[1:2], g[1:2]), (p[1], g[1])):
        ob, gb = loss.l1_ssim_value_and_grad(a, b, 0.2, per_image=True)
        assert tuple(ob.shape) == (1, 3) and torch.equal(ob[0], o0) and torch.equal(gb.reshape(g0.shape), g0)
    s_each, s_all = loss.ssim(p, g, size_average=False), loss.ssim(p, g, size_average=True)
    np.testing.assert_allclose(s_each.mean().item(), s_all.item(), rtol=2e-6)
    # the default is what it was
    o_def, g_def = loss.l1_ssim_value_and_grad(p, g, 0.2)
    assert tuple(o_def.shape) == (3,)
    np.testing.assert_allclose(o_def[0].item(), out[:, 0].mean().item(), rtol=2e-6)


@pytest.mark.gpu
def test_gpu_new_functions_are_reproducible():
    from youreditableavatar_amd import loss
    from youreditableavatar_amd.loss import _lib
    pred, gt = _inputs((4, 3, 200, 300), seed=5)
    a, b = torch.tensor(pred).cuda(), torch.tensor(gt).cuda()
    w = torch.tensor([0.5, 2.0, 1.25, 0.75]).cuda()

    def autograd(fn, upstream):
        p = a.clone().requires_grad_(True)
        v = fn(p, b)
        (v * upstream).sum().backward()
        return v.detach(), p.grad

    calls = [lambda: autograd(loss.l2_loss, 1.5), lambda: autograd(lambda x, y: loss.ssim(x, y, size_average=False), w),
             lambda: loss.l1_ssim_value_and_grad(a, b, 0.2, per_image=True), lambda: loss.pixel_value_and_grad(a, b, "l2"),
             lambda: loss.pixel_value_and_grad(a, b, "l1"), lambda: loss.pixel_value_and_grad(a, b, "l2", per_image=True),
             lambda: loss.pixel_value_and_grad(a, b, "l1", per_image=True)]
    for i, call in enumerate(calls):
        (v1, g1), (v2, g2) = call(), call()
        assert torch.equal(v1, v2) and torch.equal(g1, g2), i
    p = a.clone().requires_grad_(True)
    z = loss.l2_loss(p, a)
    z.backward()
    assert z.item() == 0.0 and torch.all(p.grad == 0)
    v, g0 = loss.pixel_value_and_grad(a, a, "l1", per_image=True)
    assert torch.all(v == 0) and torch.all(g0 == 0)
    assert loss.pixel_value_and_grad(a, b, "l2", need_grad=False)[1] is None
    # C level: one scalar upstream is the per-image upstream with that value in every entry, and NULL is 1
    B, Cn, H, W = a.shape
    nbytes = int(_lib.tgs_l1_ssim_images_workspace_bytes(B, Cn, H, W))
    ws, out = torch.empty(nbytes, dtype=torch.uint8).cuda(), torch.empty(B, 3).cuda()
    st = torch.cuda.current_stream().cuda_stream
    g_sum = torch.empty_like(a)
    assert _lib.tgs_l1_ssim_images(st, B, Cn, H, W, a.data_ptr(), b.data_ptr(), 0.2, out.data_ptr(), g_sum.data_ptr(), ws.data_ptr(), nbytes) == 0
    grads = []
    for up, per in ((torch.full((1,), 0.375).cuda(), 0), (torch.full((B,), 0.375).cuda(), 1), (None, 0), (torch.ones(B).cuda(), 1)):
        gi = torch.empty_like(a)
        assert _lib.tgs_l1_ssim_images_backward(st, B, Cn, H, W, a.data_ptr(), b.data_ptr(), 0.2, up.data_ptr() if up is not None else None, per, gi.data_ptr(),
                                                ws.data_ptr(), nbytes) == 0
        grads.append(gi)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[2], grads[3]) and torch.equal(grads[2], g_sum)
    assert not torch.equal(grads[0], grads[2])


@pytest.mark.gpu
def test_gpu_ssim_argument_errors():
    from youreditableavatar_amd import loss
    x = torch.rand(3, 16, 16).cuda()
    with pytest.raises(IndexError, match="B,C,H,W"):           # the reference's mean(1).mean(1).mean(1) of a 3-D map fails the same way
        loss.ssim(x, x, size_average=False)
    with pytest.raises(NotImplementedError):
        loss.ssim(x, x, window_size=7)
    with pytest.raises(NotImplementedError):
        loss.ssim(x[None], x[None], window_size=7, size_average=False)


@pytest.mark.gpu
def test_gpu_three_loss_settings_run():
    """the trainers' loss_function block (refine.py:241-247) on the package's functions"""
    from youreditableavatar_amd.loss import l1_loss, l2_loss, ssim
    pred, gt = _inputs((1, 3, 64, 80), seed=2)
    g = torch.tensor(gt).cuda()
    dssim_factor = 0.2
    fns = {"l1": l1_loss, "l2": l2_loss, "l1+dssim": lambda a, b: (1.0 - dssim_factor) * l1_loss(a, b) + dssim_factor * (1.0 - ssim(a, b))}
    refs = {"l1": loss_ref.l1_loss, "l2": ref_l2, "l1+dssim": lambda a, b: loss_ref.l1_ssim_loss(a, b, dssim_factor)}
    for setting, fn in fns.items():
        p = torch.tensor(pred).cuda().requires_grad_(True)
        v = fn(p, g)
        v.backward()
        p64 = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
        want = refs[setting](p64, torch.tensor(gt, dtype=torch.float64))
        (dwant,) = torch.autograd.grad(want, p64)
        np.testing.assert_allclose(v.item(), want.item(), rtol=1e-5)
        assert util.rel_l2(p.grad.cpu().numpy(), dwant.numpy()) <= 1e-5, setting


@pytest.mark.gpu
def test_run_views_with_pointwise_upstream(gpu_device):
    """SyncFreeBatch.run_views fed by pixel_value_and_grad("l2") == the same step through GaussianRasterizer + l2_loss(...).backward():
    the two paths tests/test_gpu_api.py::test_run_views_whole_batch_path compares, with its tolerance."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    from tests.test_gpu_api import _leaves, _settings
    from youreditableavatar_amd import loss, scenes
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
    P, V = 6000, 4
    cloud = scenes.make_cloud(P, 3, seed=41, scale_mult=3.0)
    cams = [scenes.orbit_camera(176, 112, azimuth_deg=a) for a in (0.0, 70.0, 140.0, 210.0)]
    gt = torch.rand(V, 3, 112, 176, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    names = ("means3D", "opacities", "scales", "rotations", "shs")
    settings = [_settings(c, 3, gpu_device) for c in cams]
    _C.set_deterministic(True)
    try:
        A = _leaves(cloud, gpu_device)
        values = []
        for v in range(V):
            img, _ = GaussianRasterizer(settings[v])(means3D=A["means3D"], means2D=torch.zeros(P, 3, device=gpu_device, requires_grad=True), shs=A["shs"],
                                                     colors_precomp=None, opacities=A["opacities"], scales=A["scales"], rotations=A["rotations"], cov3D_precomp=None)
            value = loss.l2_loss(img, gt[v])
            value.backward()
            values.append(value.item())
        B = _leaves(cloud, gpu_device)
        flat = FlatGradients([B[n] for n in names])
        batch = SyncFreeBatch(granule=256, streams=2)
        seen = []

        def upstream(images):
            value, grad = loss.pixel_value_and_grad(images, gt, "l2", per_image=True)
            seen.append(value)
            return grad

        for rep in range(2):                                    # first batch: synchronous frames; then the whole-batch path
            flat.zero_()
            batch.run_views(settings, B["means3D"], B["opacities"], B["shs"], B["scales"], B["rotations"], upstream)
            np.testing.assert_allclose(seen[-1].cpu().numpy(), np.array(values), rtol=1e-5)
            for n in names:
                assert util.rel_l2(B[n].grad.cpu().numpy(), A[n].grad.cpu().numpy()) <= 2e-5, (rep, n)
        assert batch.rejected == 0
    finally:
        _C.set_deterministic(False)
