"""GPU time of the loss module's value + gradient at the trainers' image sizes, at the C boundary (include/tgs_raster.h), so that an older
build of the library can run next to this one:

    python tools/loss_times.py [--parent-lib PATH] [--rounds 25] [--inner 10] [--check]

Operations (each is the native calls the Python function of that name makes for value AND gradient, on preallocated buffers):
    l2_loss                    tgs_pixel_loss (value) + tgs_pixel_loss_backward (upstream scalar)          reads 4 floats / element, writes 1
    pixel_l1                   tgs_pixel_loss(TGS_LOSS_L1, dL_dimg): pixel_value_and_grad("l1")             reads 2, writes 1
    l1_loss                    tgs_l1_ssim(f = 0) + tgs_l1_ssim_backward: today's l1_loss
    l1_ssim_loss               tgs_l1_ssim(f = 0.2) + tgs_l1_ssim_backward
    l1_ssim_value_and_grad     tgs_l1_ssim(f = 0.2, dL_dimg)
    l1_ssim_per_image          tgs_l1_ssim_images(f = 0.2, dL_dimg): per_image=True
Device events; every shape and operation is warmed up; `rounds` rounds, in each of which every (operation, library) pair is timed once over
`inner` back-to-back repetitions (rounds x inner >= 200 timed repetitions), the libraries alternating inside a round; medians over the
rounds.  With --parent-lib the operations the older library has run from it too, TWICE ("parent", "parent_again"): the distance between
those two is the spread any old-against-new difference has to exceed.  Prints a table and one JSON line.  Profiler off."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = ((1, 3, 1080, 1920), (1, 3, 2048, 2048), (8, 3, 1080, 1920))
COPY_CEILING = 6.29e12          # B/s: the chip's measured copy rate DESIGN.md prices the HBM-bound kernels against
VP, IT, I64, FL, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
SIGNATURES = {
    "tgs_l1_ssim_workspace_bytes": (SZ, [IT, IT, IT]),
    "tgs_l1_ssim": (IT, [VP, IT, IT, IT, VP, VP, FL, VP, VP, VP, SZ]),
    "tgs_l1_ssim_backward": (IT, [VP, IT, IT, IT, VP, VP, FL, VP, VP, VP, SZ]),
    "tgs_l1_ssim_images": (IT, [VP, IT, IT, IT, IT, VP, VP, FL, VP, VP, VP, SZ]),
    "tgs_pixel_loss_workspace_bytes": (SZ, [IT, I64]),
    "tgs_pixel_loss": (IT, [VP, IT, IT, I64, VP, VP, VP, VP, VP, SZ]),
    "tgs_pixel_loss_backward": (IT, [VP, IT, IT, I64, VP, VP, VP, IT, VP]),
}


def bind(lib):
    """-> the names of SIGNATURES this build exports, with their ctypes signatures set"""
    have = set()
    for name, (res, args) in SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
            have.add(name)
    return have


def operations(lib, have, B, Cn, H, W, img, gt, grad, out, ws, up):
    st = torch.cuda.current_stream().cuda_stream
    P, n, nb = B * Cn, Cn * H * W, ws.numel()
    a, b, g, o, w, u = img.data_ptr(), gt.data_ptr(), grad.data_ptr(), out.data_ptr(), ws.data_ptr(), up.data_ptr()

    def ok(r):
        if r != 0:
            raise RuntimeError(f"native call failed: {r}")

    def l1_ssim_autograd(f):
        return lambda: (ok(lib.tgs_l1_ssim(st, P, H, W, a, b, f, o, None, w, nb)), ok(lib.tgs_l1_ssim_backward(st, P, H, W, a, b, f, u, g, w, nb)))

    ops = {"l1_loss": l1_ssim_autograd(0.0), "l1_ssim_loss": l1_ssim_autograd(0.2),
           "l1_ssim_value_and_grad": lambda: ok(lib.tgs_l1_ssim(st, P, H, W, a, b, 0.2, o, g, w, nb))}
    if "tgs_l1_ssim_images" in have:
        ops["l1_ssim_per_image"] = lambda: ok(lib.tgs_l1_ssim_images(st, B, Cn, H, W, a, b, 0.2, o, g, w, nb))
    if "tgs_pixel_loss" in have:
        ops["l2_loss"] = lambda: (ok(lib.tgs_pixel_loss(st, 1, 1, B * n, a, b, o, None, w, nb)), ok(lib.tgs_pixel_loss_backward(st, 1, 1, B * n, a, b, u, 0, g)))
        ops["pixel_l1"] = lambda: ok(lib.tgs_pixel_loss(st, 0, 1, B * n, a, b, o, g, w, nb))
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="an older build of libtgs_raster.so to time next to this one")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--check", action="store_true", help="also compare tgs_l1_ssim's outputs between the two libraries (torch.equal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from youreditableavatar_amd.loss import _lib as new_lib
    libs = {"new": new_lib}
    if args.parent_lib:
        libs["parent"] = libs["parent_again"] = C.CDLL(os.path.abspath(args.parent_lib))
    have = {k: bind(v) for k, v in libs.items()}
    result = {"rounds": args.rounds, "inner": args.inner, "shapes": {}}
    for (B, Cn, H, W) in SHAPES:
        torch.manual_seed(1)
        gt = torch.rand(B, Cn, H, W, device="cuda")
        img = (gt + 0.1 * torch.randn_like(gt)).clamp_(0, 1)
        grad, out, up = torch.empty_like(img), torch.empty(B, 3, device="cuda"), torch.full((1,), 1.5, device="cuda")
        nbytes = max(int(new_lib.tgs_l1_ssim_workspace_bytes(B * Cn, H, W)), int(new_lib.tgs_pixel_loss_workspace_bytes(1, B * Cn * H * W)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ops = {k: operations(v, have[k], B, Cn, H, W, img, gt, grad, out, ws, up) for k, v in libs.items()}
        pairs = [(op, k) for op in ops["new"] for k in libs if op in ops[k]]
        for op, k in pairs:                                        # warm-up: code objects loaded, clocks up
            for _ in range(args.inner):
                ops[k][op]()
        torch.cuda.synchronize()
        events = {p: [] for p in pairs}
        for _ in range(args.rounds):
            for p in pairs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(args.inner):
                    ops[p[1]][p[0]]()
                e1.record()
                events[p].append((e0, e1))
        torch.cuda.synchronize()
        times = {p: sorted(e0.elapsed_time(e1) * 1e3 / args.inner for e0, e1 in ev) for p, ev in events.items()}
        shape = "x".join(str(s) for s in (B, Cn, H, W))
        entry = {}
        for op in ops["new"]:
            entry[op] = {k: {"median_us": round(statistics.median(times[(op, k)]), 2), "min_us": round(times[(op, k)][0], 2)} for k in libs if (op, k) in times}
        elems = B * Cn * H * W
        for op, floats in (("l2_loss", 5), ("pixel_l1", 3)):       # what the passes move: 2 reads (+ 2 reads + 1 write) of 4 bytes per element
            rate = floats * 4 * elems / (entry[op]["new"]["median_us"] * 1e-6)
            entry[op]["bytes_per_s"] = round(rate / 1e12, 3)
            entry[op]["of_copy_ceiling"] = round(rate / COPY_CEILING, 3)
        result["shapes"][shape] = entry
        print(f"--- {shape}: median (min) us per value + gradient over {args.rounds} x {args.inner} repetitions")
        for op, e in entry.items():
            line = "  ".join(f"{k} {e[k]['median_us']:8.2f} ({e[k]['min_us']:8.2f})" for k in libs if k in e)
            extra = f"   {e['bytes_per_s']} TB/s = {e['of_copy_ceiling']} of the copy ceiling" if "bytes_per_s" in e else ""
            print(f"{op:24s} {line}{extra}")
        if args.check and args.parent_lib:
            outs = []
            for k in ("new", "parent"):
                o, g = torch.empty(3, device="cuda"), torch.empty_like(img)
                r = libs[k].tgs_l1_ssim(torch.cuda.current_stream().cuda_stream, B * Cn, H, W, img.data_ptr(), gt.data_ptr(), 0.2, o.data_ptr(), g.data_ptr(), ws.data_ptr(), nbytes)
                assert r == 0
                outs.append((o, g))
            same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            result["shapes"][shape]["tgs_l1_ssim_equal_to_parent"] = same
            print("tgs_l1_ssim out3 and dL_dimg equal to the parent's:", same)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
