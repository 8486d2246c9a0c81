"""Time of optimizer.step() over the Gaussian parameter groups of the config-3 cloud (500 k Gaussians), and of the trainers' per-step protocol
(tools/trainer_protocol.py's loop, copied here) with each optimizer appended:

    python tools/optim_times.py [--rounds 7] [--inner 200] [--protocol-steps 30]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rp -- python tools/optim_times.py --profile OPT DEG LAYOUT [--steps 20]
    python tools/optim_times.py --summarize DIR [--steps 20]

Optimizers:  torch_default  torch.optim.Adam(l, lr=0.0, eps=1e-15): what the reference runs (tetgs_optimizer.py:92), torch's foreach path on a device
             torch_fused    the same with fused=True
             fused_adam     youreditableavatar_amd.optim.FusedAdam (csrc/tgs_optim.hip: one launch per step)
Cases:       SH degree 0 (points, dc, densities, scales, quaternions: 14 floats per Gaussian) and degree 3 (+ the 15 rest coefficients: 59),
             the gradients contiguous or level-major (multiview.FlatGradients(level_major=True): the SH parameters' .grad is a strided view of
             coefficient planes).  An optimizer that refuses a case is reported with its message, not timed.

Method: every (case, optimizer) pair is warmed up; then `rounds` rounds, in each of which every optimizer of the case runs `inner` steps between
two device events, the optimizers alternating inside a round (rounds x inner timed steps each).  Reported: median, min and max of the rounds'
ms per step (max - min is the spread a difference has to exceed), the bytes a 7-pass step moves (28 per parameter float) over the median and
that rate's share of the 6.29 TB/s copy ceiling.  The time is what a trainer sees per step(): the GPU time of the step's kernels, or the host's
time to enqueue them where that is longer.  Profiler off; kernel counts come from the --profile runs.  Prints tables and one JSON line."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_CEILING = 6.29e12          # B/s: the chip's measured copy rate DESIGN.md prices the HBM-bound kernels against
OPTIMIZERS = ("torch_default", "torch_fused", "fused_adam")
RATES = {"points": 0.00016, "sh_coordinates_dc": 0.0025, "sh_coordinates_rest": 0.0025 / 20.0, "all_densities": 0.05, "scales": 0.005, "quaternions": 0.001}


def make_optimizer(kind, groups):
    from youreditableavatar_amd.optim import FusedAdam
    if kind == "torch_default":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if kind == "torch_fused":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True)
    return FusedAdam(groups, lr=0.0, eps=1e-15)


def model_parameters(cloud, deg, dev):
    """the model's raw parameters under the optimizer's group names (tetgs_model.py:196-239), as tools/trainer_protocol.py builds them"""
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).requires_grad_(True)
    op = np.clip(cloud["opacities"], 1e-4, 1 - 1e-4)
    L = {"points": g(cloud["means3D"]), "sh_coordinates_dc": g(cloud["shs"][:, :1])}
    if deg > 0:
        L["sh_coordinates_rest"] = g(cloud["shs"][:, 1:])
    L.update(all_densities=g(np.log(op / (1 - op))), scales=g(np.log(cloud["scales"])), quaternions=g(cloud["rotations"]))
    return L


def groups_of(L):
    return [{"params": [p], "lr": RATES[n], "name": n} for n, p in L.items()]


def optimizer_case(cloud, deg, level_major, kind, dev):
    """-> (optimizer, floats per step) over its own copy of the parameters, every .grad a view of one FlatGradients buffer filled with noise"""
    from youreditableavatar_amd.multiview import FlatGradients
    L = model_parameters(cloud, deg, dev)
    names = list(L)
    sh = {names.index("sh_coordinates_dc"): 0}
    if deg > 0:
        sh[names.index("sh_coordinates_rest")] = 1
    flat = FlatGradients([L[n] for n in names], sh_params=sh, level_major=level_major)
    gen = torch.Generator(device=dev).manual_seed(7)
    for p in L.values():
        p.grad.copy_(torch.randn(p.shape, generator=gen, device=dev) * 1e-3)
    opt = make_optimizer(kind, groups_of(L))
    opt._keep = (L, flat)
    return opt, sum(p.numel() for p in L.values())


def time_optimizers(cloud, dev, rounds, inner):
    out = {}
    for deg in (0, 3):
        for level_major in (False, True):
            case = f"sh{deg}_{'level_major' if level_major else 'contiguous'}"
            opts, entry, floats = {}, {}, 0
            for kind in OPTIMIZERS:
                opt, floats = optimizer_case(cloud, deg, level_major, kind, dev)
                try:                                               # warm-up; an optimizer that refuses the layout says so here
                    for _ in range(10):
                        opt.step()
                    torch.cuda.synchronize()
                    opts[kind] = opt
                except Exception as e:                             # noqa: BLE001
                    entry[kind] = {"refused": f"{type(e).__name__}: {str(e).splitlines()[0][:200]}"}
            events = {k: [] for k in opts}
            host = {k: [] for k in opts}
            for _ in range(rounds):
                for k, opt in opts.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _i in range(inner):
                        opt.step()
                    e1.record()
                    host[k].append((time.perf_counter() - t0) / inner * 1e3)
                    torch.cuda.synchronize()
                    events[k].append(e0.elapsed_time(e1) / inner)
            for k in opts:
                ms = sorted(events[k])
                med = statistics.median(ms)
                rate = 28 * floats / (med * 1e-3)
                entry[k] = {"median_ms": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "host_enqueue_ms": round(statistics.median(host[k]), 4),
                            "seven_pass_TB_per_s": round(rate / 1e12, 3), "of_copy_ceiling": round(rate / COPY_CEILING, 3)}
            out[case] = {"parameter_floats": floats, "seven_pass_MB": round(28 * floats / 1e6, 1), **entry}
            print(f"--- {case}: {floats} parameter floats, a 7-pass step moves {28 * floats / 1e6:.1f} MB; ms per step() over {rounds} x {inner} steps: median (min .. max), host enqueue")
            for k in OPTIMIZERS:
                e = entry[k]
                print(f"{k:14s} " + (f"refused: {e['refused']}" if "refused" in e else
                                     f"{e['median_ms']:8.4f} ({e['min_ms']:.4f} .. {e['max_ms']:.4f})  host {e['host_enqueue_ms']:.4f}   "
                                     f"{e['seven_pass_TB_per_s']} TB/s of 7-pass bytes = {e['of_copy_ceiling']} of the copy ceiling"))
            del opts
            torch.cuda.empty_cache()
    return out


def protocol_steps(cloud, deg, dev, kinds, rounds, steps):
    """tools/trainer_protocol.py's step (bindings -> SH colours -> rasterizer at 2048 x 2048 -> L1 + SSIM loss -> backward) followed by
    optimizer.step(); `none`: that tool's loop as it is.  -> {kind: ms per step of each round}"""
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.bindings import gaussian_bind
    from youreditableavatar_amd.loss import l1_ssim_loss
    from youreditableavatar_amd.sh_color import points_rgb_dc_rest
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    W = H = 2048
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    S = []
    for k in range(16):
        c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
        S.append(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg), scale_modifier=1.0, viewmatrix=g(c.viewmatrix),
                                               projmatrix=g(c.projmatrix), sh_degree=deg, campos=g(c.campos), prefiltered=False, debug=False))
    gt = torch.rand(3, H, W, device=dev)
    P = cloud["means3D"].shape[0]
    state = {}
    for kind in kinds:
        L = model_parameters(cloud, deg, dev)
        state[kind] = (L, None if kind == "none" else make_optimizer(kind, groups_of(L)), [0])

    def step(kind):
        L, opt, count = state[kind]
        rs = S[count[0] % len(S)]
        count[0] += 1
        for t in L.values():
            t.grad = None
        colors = points_rgb_dc_rest(L["sh_coordinates_dc"], L.get("sh_coordinates_rest"), deg + 1, positions=L["points"], camera_centers=rs.campos)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        opacities, scales, rotations, _ = gaussian_bind(L["all_densities"], L["scales"], L["quaternions"])
        img, _ = GaussianRasterizer(rs)(means3D=L["points"], means2D=m2, opacities=opacities, colors_precomp=colors, scales=scales, rotations=rotations)
        l1_ssim_loss(img, gt, 0.2).backward()
        if opt is not None:
            opt.step()

    for kind in kinds:
        for _ in range(10):
            step(kind)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(rounds):
        for kind in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _i in range(steps):
                step(kind)
            torch.cuda.synchronize()
            times[kind].append((time.perf_counter() - t0) / steps * 1e3)
    return times


def time_protocol(cloud, dev, rounds, steps):
    out = {}
    kinds = ("none",) + OPTIMIZERS
    for deg in (0, 3):
        times = protocol_steps(cloud, deg, dev, kinds, rounds, steps)
        entry = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}
        out[f"sh{deg}"] = entry
        print(f"--- trainers' step at 2048 x 2048, SH degree {deg}, ms per step over {rounds} x {steps} steps: median (min .. max); 'none' = tools/trainer_protocol.py")
        for k in kinds:
            e = entry[k]
            print(f"{k:14s} {e['median_ms']:8.4f} ({e['min_ms']:.4f} .. {e['max_ms']:.4f})   + {e['median_ms'] - entry['none']['median_ms']:.4f} over the step without an optimizer")
    return out


def summarize(directory, steps):
    """kernels per step() out of a --profile run's rocprofv3 statistics: every kernel called at least once per step"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    if not rows:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    per_step = [(n, c / steps, t / steps / 1e3) for n, c, t in rows if c >= steps]
    print(f"{directory}: {sum(c for _n, c, _t in per_step):.1f} kernel launches and {sum(t for _n, _c, t in per_step):.1f} us of kernel time per step()")
    for n, c, t in sorted(per_step, key=lambda x: -x[2]):
        print(f"  {c:5.1f} x  {t:8.1f} us  {n[:150]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--protocol-steps", type=int, default=30)
    ap.add_argument("--profile", nargs=3, metavar=("OPT", "DEG", "LAYOUT"), help="run `--steps` steps of one optimizer on one case and exit (for rocprofv3)")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.steps)
    assert torch.cuda.is_available(), "needs a HIP device"
    if args.rounds < 5:
        raise SystemExit("at least five rounds: the spread of the rounds is what a difference is measured against")
    from youreditableavatar_amd import scenes
    dev = torch.device("cuda", 0)
    cloud = scenes.config_cloud(3)
    if args.profile:
        kind, deg, layout = args.profile
        opt, _ = optimizer_case(cloud, int(deg), layout == "level_major", kind, dev)
        for _ in range(args.steps):
            opt.step()
        torch.cuda.synchronize()
        return
    result = {"gaussians": int(cloud["means3D"].shape[0]), "rounds": args.rounds, "inner": args.inner,
              "optimizer_step": time_optimizers(cloud, dev, args.rounds, args.inner),
              "trainer_protocol": time_protocol(cloud, dev, max(args.rounds, 5), args.protocol_steps)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
