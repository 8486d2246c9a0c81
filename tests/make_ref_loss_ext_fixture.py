#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Imports the reference's Edit_core/utils/loss_utils.py from /root/reference and records into
tests/golden/ref_loss_ext_fixture.npz what tests/make_ref_loss_fixture.py leaves out: its l2_loss with the autograd
gradient, and ssim(size_average=False) on [B,C,H,W] batches with the gradient of (ssim * w).sum() for a recorded
non-uniform weight vector w[B] (a per-image upstream that is mixed up between images cannot pass).  Also the names the
reference's three trainers import from utils.loss_utils, read from their import lines.  A fixture is data; no
reference source is copied.

Every case is evaluated in float64 as well (oracle/loss_ref.py); the fixture stores the reference's distance from it,
and a case whose recorded fp32 gradient is further than 1e-5 rel-L2 from the float64 one is refused (one-channel
convolution backward on the CPU differs between machines: see oracle/loss_ref.py)."""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import loss_ref  # noqa: E402

REF = "/root/reference/Edit_core"
OUT = os.path.join(HERE, "golden", "ref_loss_ext_fixture.npz")
TRAINERS = ("tetgs_texture/refine.py", "tetgs_texture/refine_3dgs.py", "tetgs_texture/paint_2dgs.py")
SSIM_CASES = {"a": (2, 3, 37, 53), "b": (4, 1, 9, 70), "c": (1, 3, 16, 16), "d": (3, 3, 64, 96)}
L2_CASES = {"e": (1, 1, 1), "f": (3, 7, 11), "g": (3, 16, 16)}          # 3-D: one pixel; 231 elements (not a multiple of 4); a small image
GRAD_CAP = 1e-5


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def inputs(rng, shape):
    # 8-bit levels, as a target image read from a file has them: the arrays compress to a quarter, which keeps the fixture small
    gt = (rng.integers(0, 256, shape) / 255.0).astype(np.float32)
    pred = (np.round(np.clip(gt + rng.normal(0, 0.15, shape), 0, 1) * 255.0) / 255.0).astype(np.float32)
    if pred.size > 1:
        pred[..., ::5, ::7] = gt[..., ::5, ::7]                # exact matches: a zero gradient of l2, sign(0) of l1
    return pred, gt


def trainer_imports():
    names = []
    for t in TRAINERS:
        found = False
        for line in open(os.path.join(REF, t)):
            m = re.match(r"\s*from\s+utils\.loss_utils\s+import\s+(.+)", line)
            if m:
                found = True
                names += [n.strip() for n in m.group(1).split("#")[0].split(",") if n.strip()]
        assert found, t
    return sorted(set(names))


def main():
    sys.path.insert(0, REF)
    from utils import loss_utils as lu
    rng = np.random.Generator(np.random.PCG64(23))
    out, report = {}, []
    for name, shape in {**SSIM_CASES, **L2_CASES}.items():
        pred, gt = inputs(rng, shape)
        p, g = torch.tensor(pred, requires_grad=True), torch.tensor(gt)
        p64, g64 = torch.tensor(pred, dtype=torch.float64, requires_grad=True), torch.tensor(gt, dtype=torch.float64)
        case = {f"{name}_pred": pred, f"{name}_gt": gt}
        v = lu.l2_loss(p, g)
        (dv,) = torch.autograd.grad(v, p)
        v64 = ((p64 - g64) ** 2).mean()
        (dv64,) = torch.autograd.grad(v64, p64)
        dist = [abs(v.item() - v64.item()) / abs(v64.item()), rel_l2(dv.numpy(), dv64.numpy())]
        case.update({f"{name}_l2": v.detach().numpy(), f"{name}_dl2": dv.numpy()})
        if name in SSIM_CASES:
            w = rng.uniform(0.25, 2.0, shape[0]).astype(np.float32)
            s = lu.ssim(p, g, size_average=False)
            assert tuple(s.shape) == (shape[0],)
            (ds,) = torch.autograd.grad((s * torch.tensor(w)).sum(), p)
            s64 = loss_ref.ssim_map(p64, g64).mean((-3, -2, -1))
            (ds64,) = torch.autograd.grad((s64 * torch.tensor(w, dtype=torch.float64)).sum(), p64)
            dist += [float(np.max(np.abs(s.detach().numpy() - s64.detach().numpy()) / np.abs(s64.detach().numpy()))), rel_l2(ds.numpy(), ds64.numpy())]
            case.update({f"{name}_w": w, f"{name}_ssim": s.detach().numpy(), f"{name}_dssim": ds.numpy()})
        case[f"{name}_fp64_distance"] = np.array(dist)            # (l2 value, l2 gradient[, ssim values, ssim gradient]) of the reference from float64
        report.append((name, shape, dist))
        if max(dist[1::2]) > GRAD_CAP:
            print(f"REFUSED case {name} {shape}: fp32 gradient {max(dist[1::2]):.3g} rel-L2 from float64 (> {GRAD_CAP})")
            continue
        out.update(case)
    # the [C,H,W] form of size_average=False fails in the reference itself: record how
    try:
        lu.ssim(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16), size_average=False)
        out["ssim_3d_per_image_error"] = np.array("")
    except Exception as e:                                        # noqa: BLE001
        out["ssim_3d_per_image_error"] = np.array(type(e).__name__)
    out["trainer_imports"] = np.array(trainer_imports())
    out["cases_ssim"] = np.array([k for k in SSIM_CASES if f"{k}_pred" in out])
    out["cases_l2"] = np.array([k for k in {**SSIM_CASES, **L2_CASES} if f"{k}_pred" in out])
    np.savez_compressed(OUT, **out)
    for name, shape, dist in report:
        print(name, shape, " ".join(f"{d:.3g}" for d in dist))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", list(out["trainer_imports"]), str(out["ssim_3d_per_image_error"]))


if __name__ == "__main__":
    main()
