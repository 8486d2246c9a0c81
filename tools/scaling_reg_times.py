"""What the scaling regulariser of the refinement loops (tetgs_texture/refine.py:306-317) costs per step, on the trainers' per-step protocol
(tools/trainer_protocol.py's loop at 2048 x 2048 on the config-3 cloud, copied here as tools/optim_times.py copies it) with FusedAdam appended:

    python tools/scaling_reg_times.py [--rounds 7] [--steps 100]

Variants:  none    the step without the regulariser
           torch   the reference's lines written in torch: torch.max / torch.min over the bound scaling, the ratio, the two comparisons, the
                   boolean gather, `if thresh_idxs.sum() > 0:` (a host read-back) and the mean -- with the radii CACHED, which is kinder than
                   the reference (tetgs.radii rebuilds them from the mesh on every access, tetgs_model.py:299-310)
           fused   regularizers.scaling_regularizer_raw on the raw scales (csrc/tgs_reg.hip: two launches forward, one backward, no read-back)
Cases:     SH degree 0 and 3.

The radii stand in for a mesh: the largest scale of every Gaussian times a factor in [0.5, 2], so that about half of the rows exceed their
radius, and every other Gaussian carries the flat axis of a mesh-bound one (log(1e-8), tetgs_edit_2d.py:203): the term is live at every step.

Method (tools/optim_times.py's): every variant is warmed up; then `rounds` rounds, in each of which every variant runs `steps` steps between two
device events, the variants alternating inside a round.  Reported: median and (min .. max) of the rounds' ms per step, and each
regulariser's added cost over `none` -- a difference between two variants counts when it exceeds the (min .. max) spreads.  Profiler off.
Prints the tables and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

VARIANTS = ("none", "torch", "fused")
RATES = {"points": 0.00016, "sh_coordinates_dc": 0.0025, "sh_coordinates_rest": 0.0025 / 20.0, "all_densities": 0.05, "scales": 0.005, "quaternions": 0.001}


def torch_lines(scaling, radii):
    """refine.py:308-317 as the trainer runs them -> the term, or None when the loop adds nothing"""
    thresh_scaling_max = radii * 1.0
    max_vals, _ = torch.max(scaling, dim=-1)
    min_vals, _ = torch.min(scaling, dim=-1)
    ratio = max_vals / min_vals
    thresh_idxs = (max_vals > thresh_scaling_max) & (ratio > 10.0)
    if thresh_idxs.sum() > 0:
        return max_vals[thresh_idxs].mean() * 1.0
    return None


def run(cloud, deg, dev, rounds, steps):
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.bindings import gaussian_bind
    from youreditableavatar_amd.loss import l1_ssim_loss
    from youreditableavatar_amd.optim import FusedAdam
    from youreditableavatar_amd.regularizers import scaling_regularizer_raw
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
    rng = np.random.default_rng(17)
    radii = g(cloud["scales"].max(axis=1) * np.exp(rng.uniform(-0.7, 0.7, P)))
    op = np.clip(cloud["opacities"], 1e-4, 1 - 1e-4)
    state, selected = {}, {}
    for kind in VARIANTS:
        p = lambda x: g(x).requires_grad_(True)
        L = {"points": p(cloud["means3D"]), "sh_coordinates_dc": p(cloud["shs"][:, :1])}
        if deg > 0:
            L["sh_coordinates_rest"] = p(cloud["shs"][:, 1:])
        L.update(all_densities=p(np.log(op / (1 - op))), scales=p(np.log(cloud["scales"])), quaternions=p(cloud["rotations"]))
        state[kind] = (L, FusedAdam([{"params": [t], "lr": RATES[n], "name": n} for n, t in L.items()], lr=0.0, eps=1e-15), [0])

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
        loss = l1_ssim_loss(img, gt, 0.2)
        if kind == "torch":
            term = torch_lines(scales, radii)
            if term is not None:
                loss = loss + term
        elif kind == "fused":
            loss = loss + scaling_regularizer_raw(L["scales"], radii)
        loss.backward()
        opt.step()

    # the same flat axis in every variant's parameters (the regularised variants then move their scales; `none` does not: the rasterizer sees
    # slightly different clouds after the warm-up, which is what a trainer with and without the term sees as well)
    for kind in VARIANTS:
        with torch.no_grad():
            state[kind][0]["scales"][::2, 0] = float(np.log(1e-8))
    for kind in VARIANTS:
        for _ in range(10):
            step(kind)
    torch.cuda.synchronize()
    for kind in ("torch", "fused"):
        with torch.no_grad():
            _, codes = scaling_regularizer_raw(state[kind][0]["scales"].detach(), radii, return_codes=True)
            selected[kind] = int((codes != 0).sum())
    times = {k: [] for k in VARIANTS}
    for _ in range(rounds):
        for kind in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _i in range(steps):
                step(kind)
            e1.record()
            torch.cuda.synchronize()
            times[kind].append(e0.elapsed_time(e1) / steps)
    return times, selected, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    if args.rounds < 5:
        raise SystemExit("at least five rounds: the spread of the rounds is what a difference is measured against")
    from youreditableavatar_amd import scenes
    dev = torch.device("cuda", 0)
    cloud = scenes.config_cloud(3)
    out = {}
    for deg in (0, 3):
        times, selected, P = run(cloud, deg, dev, args.rounds, args.steps)
        entry = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}
        none = entry["none"]["median_ms"]
        print(f"--- trainers' step + FusedAdam at 2048 x 2048, {P} Gaussians, SH degree {deg}; rows selected after the warm-up: {selected}; "
              f"ms per step over {args.rounds} x {args.steps} steps: median (min .. max)")
        for k in VARIANTS:
            e = entry[k]
            e["added_ms"] = round(e["median_ms"] - none, 4)
            e["spread_ms"] = round(e["max_ms"] - e["min_ms"], 4)
            print(f"{k:6s} {e['median_ms']:8.4f} ({e['min_ms']:.4f} .. {e['max_ms']:.4f})   + {e['added_ms']:.4f} over the step without the regulariser")
        saved = round(entry["torch"]["added_ms"] - entry["fused"]["added_ms"], 4)
        spread = max(entry[k]["spread_ms"] for k in VARIANTS)
        print(f"       the torch lines add {entry['torch']['added_ms']:.4f} ms, the fused form {entry['fused']['added_ms']:.4f} ms: {saved:.4f} ms less; "
              f"largest (min .. max) spread of the three variants {spread:.4f} ms -> the difference {'exceeds' if saved > spread else 'does NOT exceed'} it")
        out[f"sh{deg}"] = {**entry, "selected_rows": selected, "fused_saves_ms": saved, "largest_spread_ms": spread, "exceeds_spread": bool(saved > spread)}
        torch.cuda.empty_cache()
    print(json.dumps({"gaussians": int(cloud["means3D"].shape[0]), "rounds": args.rounds, "steps": args.steps, "scaling_reg": out}))


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"(wall time {time.time() - t0:.0f} s)")
