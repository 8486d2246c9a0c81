#!/usr/bin/env python3
"""bench.py -- rasterized fragments/sec (fwd+bwd) of the MI355X-native Gaussian rasterizer.

Workload (BASELINE.json configs[2]/[3]): 500k Gaussians, 1920x1080, SH degree 3 evaluated inside the
rasterizer, orbit cameras of the 64-view batch.  A *step* = one data-parallel batch: every GPU renders
``--views-per-gpu`` (default 8 = 64 views / 8 GPUs) frames, each one forward + one backward of the
rasterizer with the upstream gradient supplied, through multiview.SyncFreeBatch.run_views (three native calls
per step, no host synchronisation per frame, views on four HIP streams, one per-Gaussian backward pass for the
batch; ``--per-view-calls`` / ``--sync-per-frame`` select the autograd path / the reference's protocol), the
per-Gaussian gradients of all views landing in one flat buffer; at N > 1 the step ends with ONE RCCL
all-reduce of that buffer (236 B/Gaussian).  Per-GPU work is fixed as N grows (weak scaling).
Metric numerator: F = sum over pixels of n_contrib, counted per view outside the
timed region.  Inputs are resident in HBM before the timed region starts.

A plain run sets up, warms up, times the K steps and prints the JSON line.  ``--full`` adds everything else the line
reports: per-kernel times and the roofline of the dominant kernel, the secondary workloads and the CPU baselines.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--config 3] [--mode sh|precomp] [--full [--no-cpu] [--no-secondary]]
       [--dump-outputs DIR]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
# VALU issue peak: 256 CUs x 4 SIMD-32 x 2.4 GHz / 2 cycles per wave64 instruction (MI355X_MICROARCH.md, cycle constants: v_fma_f32 2 cyc/SIMD)
VALU_PEAK_GWIPS = 1228.8
# measured with tools/microbench/valu_issue_rate.hip (profiles/r02_a_valu_issue_rate.txt), 8 waves per SIMD: independent v_fma_f32, and the
# render loops' mix (6 fma/mul + 1 DPP + 1 transcendental per 8: DPP operations issue at half rate, v_exp_f32 at a quarter)
VALU_MEASURED_FMA_GWIPS = 955.5
VALU_MEASURED_MIX_GWIPS = 628.4
PROFILE_SET = "r06_f"          # profiles/<set>_{hbm,sq}_counters.json: the PMC passes the roofline object quotes (tools/profile_round.sh); only
                               # used while their csrc_sha16 equals the hash of the sources this run executes (build.source_hash)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views-per-gpu", type=int, default=8, help="frames each GPU renders per step (64-view batch / 8 GPUs)")
    ap.add_argument("--config", type=int, default=3, help="BASELINE.json config index (1-based); 3 = 500k/1080p/SH3")
    ap.add_argument("--mode", default="sh", choices=["sh", "precomp"])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--split-streams", action="store_true", help="half of the streams bin, the other half composite (SyncFreeBatch(split=True))")
    ap.add_argument("--batch-upstream", action="store_true", help="dL/d images from ONE call on all images of the step (the streams meet between forwards and backwards) instead of per view on the view's stream")
    ap.add_argument("--streams", type=int, default=4, help="HIP streams the views of a step alternate between (SyncFreeBatch)")
    ap.add_argument("--loss", action="store_true", help="upstream gradient from the fused L1+SSIM loss against fixed target images (a training "
                    "step's image-space work) instead of a fixed dL/d image; not the headline metric")
    ap.add_argument("--per-view-calls", action="store_true", help="drive every view through autograd (SyncFreeBatch.run) instead of the whole-batch path (run_views)")
    ap.add_argument("--sync-per-frame", action="store_true", help="reference protocol: read num_rendered back in every forward")
    ap.add_argument("--no-fused-accumulate", action="store_true", help="let autograd add each view's gradients in a separate pass")
    ap.add_argument("--full", action="store_true", help="besides the headline: per-kernel times and the roofline (an instrumented pass before and after the timed "
                    "steps), the secondary workloads and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed (images, parameter gradients, dL/d means2D) as DIR/<name>.npy, "
                    "float32; arrays over the budget as a fixed seeded sample")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to smoke-test the N>1 control flow)")
    ap.add_argument("--same-device", action="store_true", help="testing only: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--cpu-frames", type=int, default=3)
    ap.add_argument("--order", default="random", choices=["random", "morton"], help="index order of the synthetic Gaussians: the generator's random permutation "
                    "(default, the headline) or a 3-D Morton curve (neighbours in index are neighbours in space, like mesh-bound Gaussians); not the headline")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the secondary workloads (drop-in API per frame, the trainers' protocol at 2048x2048, grown splats, "
                    "alive-pair count) that are reported beside the headline at N = 1")
    ap.add_argument("--cpu-splat-only", action="store_true", help="internal: run only the PyTorch point-splat CPU baseline of BASELINE config 1 and print its JSON "
                    "(cpu_baseline starts this as a child process with a time limit)")
    ap.add_argument("--grad-chunks", type=int, default=2, help="N > 1: the step's per-Gaussian pass runs in this many Gaussian ranges and each range's all-reduce "
                    "starts behind its launch (1 = one blocking all-reduce behind the whole pass).  Default 2 since round 4: cutting the pass costs 1 %% "
                    "with two ranges and 4.6 %% with four, a collective 13-42 us at world size 1 (secondary.rccl_world1), and the all-reduce is longer "
                    "than the whole pass -- two ranges expose the least (DESIGN.md section 7)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def launch_ranks(a) -> int:
    """``python bench.py --gpus N`` (N > 1) outside a launcher: start N ranks -- one process per GPU -- as a CHILD
    ``python -m torch.distributed.run`` with the same arguments, relay what rank 0 prints, return the child's exit code.
    Runs before anything in this process imports torch or touches the GPU; never exec()s."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main():
    a = parse()
    if a.cpu_splat_only:            # (no GPU, no distributed: a CPU-only child of cpu_baseline)
        global np
        import numpy as np
        print(json.dumps(torch_point_splat_cfg1()), flush=True)
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a))
    global np, torch
    import numpy as np
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started {world} rank(s)")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev_index = 0 if (world == 1 or a.same_device) else local_rank
    n_devices = torch.cuda.device_count()
    if dev_index >= n_devices:
        raise SystemExit(f"bench.py: rank {rank} needs cuda:{dev_index} but this node has {n_devices} GPU(s) (--same-device --backend gloo: "
                         "control-flow smoke test of N ranks on one GPU)")
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(dev_index)
        if a.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend=a.backend)
    else:
        dist = None
        torch.cuda.set_device(0)
    dev = torch.device("cuda", dev_index)
    N = world

    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch, rasterize_accumulate
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C

    cfg = dict(scenes.CONFIGS[a.config])
    P, W, H, D = cfg["P"], cfg["width"], cfg["height"], cfg["sh_degree"]
    cloud = scenes.config_cloud(a.config)
    if a.order == "morton":
        cloud = scenes.morton_order(cloud)
    dL_np = scenes.upstream_gradient(W, H, seed=cfg["seed"] + 1000)
    V = a.views
    cams = [scenes.orbit_camera(W, H, azimuth_deg=k * 360.0 / V) for k in range(V)]

    g = lambda x, rg=False: torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(rg)
    means3D, opac = g(cloud["means3D"], True), g(cloud["opacities"], True)
    scales, rots, shs = g(cloud["scales"], True), g(cloud["rotations"], True), g(cloud["shs"], True)
    params = [means3D, opac, scales, rots, shs]
    dL = g(dL_np)
    settings = []
    for c in cams:
        settings.append(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg), scale_modifier=1.0,
            viewmatrix=g(c.viewmatrix), projmatrix=g(c.projmatrix), sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False))
    colors_pre = None
    if a.mode == "precomp":
        colors_pre = [None] * V

    fused = not (a.no_fused_accumulate or a.mode != "sh")

    def rasterize(view, r_capacity=None):
        rs = settings[view]
        means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
        if fused:   # multi-view path: the backward adds into the flat gradient buffer directly (multiview.rasterize_accumulate)
            rast = lambda **kw: rasterize_accumulate(rs, r_capacity=r_capacity, return_meta=True, **kw)
        else:
            rast = GaussianRasterizer(rs)
        if a.mode == "sh":
            return rast(means3D=means3D, means2D=means2D, opacities=opac, shs=shs, scales=scales, rotations=rots)
        if colors_pre[view] is None:
            colors_pre[view] = g(scenes.sh_to_rgb_numpy(cloud["shs"], cloud["means3D"], cams[view].campos, D), True)
        return rast(means3D=means3D, means2D=means2D, opacities=opac, colors_precomp=colors_pre[view], scales=scales, rotations=rots)

    batch = SyncFreeBatch(streams=a.streams, split=a.split_streams) if (fused and not a.sync_per_frame) else None

    VPG = a.views_per_gpu

    def views_of(step):
        """contiguous shard of the step's N*VPG-view batch (multiview.shard_views), cycling through the V orbit views"""
        b0 = step * N * VPG + rank * VPG
        return [(b0 + i) % V for i in range(VPG)]

    # fragment / instance counts of the views this rank will time (outside the timed region).  F = sum of n_contrib as the
    # REFERENCE's state defines it (positions in the full 3-sigma-rectangle lists), so instance pruning is off
    # for this count; R_binned (--full) is what the timed path really bins.
    used = sorted({v for s in range(a.steps) for v in views_of(s)})
    F_view, R_view, Rb_view = {}, {}, {}
    empty = torch.Tensor([])
    for prune in ((False, True) if a.full else (False,)):
        _C.set_instance_pruning(prune)
        for v in used:
            rs = settings[v]
            R, color, radii, geom, binning, img = _C.rasterize_gaussians(rs.bg, means3D.detach(), empty, opac.detach(), scales.detach(), rots.detach(), 1.0,
                                                                       empty, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, shs.detach(), D,
                                                                       rs.campos, False, False)
            if prune:
                Rb_view[v] = int(R)
            else:
                nc = _C.state_field("n_contrib", P, W, H, R, True, True, geom, binning, img)
                F_view[v] = int(nc.to(torch.int64).sum().item())
                R_view[v] = int(R)
                del nc
            del geom, binning, img, color, radii
    _C.set_instance_pruning(True)           # (a process-wide setting) the library's default again: the timed path bins the pruned lists
    torch.cuda.synchronize()

    flat = FlatGradients(params)            # parameter .grad tensors are views of one buffer: one collective per step

    # dL/d image per view, evaluated on the view's own stream (run_views(upstream_view=...)); --batch-upstream: one call for all views
    upstream_batch, upstream_view = None, (lambda v, image: dL)
    if a.loss:
        from youreditableavatar_amd.loss import l1_ssim_value_and_grad
        # stand-ins for the ground-truth images of the step's views, seeded: the same inputs in every run
        targets = torch.rand(VPG, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(cfg["seed"] + 2000))
        upstream_view = lambda v, image: l1_ssim_value_and_grad(image[None], targets[v:v + 1])[1][0]
    if a.batch_upstream:
        upstream_view = None
        upstream_batch = (lambda images: l1_ssim_value_and_grad(images, targets)[1]) if a.loss else (lambda images: dL)

    chunks = max(1, a.grad_chunks) if (dist is not None) else 1
    pending = []

    def reduce_range(first, count):
        pending.extend(flat.all_reduce_rows(first, count))      # asynchronous, behind the launch that made this range final

    def step(s):
        """one step; returns the images it rendered (the gradients are in the parameters' .grad)"""
        if batch is not None and not a.per_view_calls:
            # three native calls per step (forward of all views, per-pixel backward of all views, one per-Gaussian backward), one Meta read-back;
            # the one per-Gaussian pass of the step STORES the gradients, so the flat buffer needs no zeroing.  N > 1: that pass runs range by
            # range and every range's all-reduce (RCCL, its own stream) runs beside the pass over the next one.
            if chunks > 1:
                images = batch.run_views([settings[v] for v in views_of(s)], means3D, opac, shs, scales, rots, upstream_batch, accumulate=False,
                                         upstream_view=upstream_view, grad_chunks=chunks, on_chunk=reduce_range)
                for w in pending:
                    w.wait()
                pending.clear()
            else:
                images = batch.run_views([settings[v] for v in views_of(s)], means3D, opac, shs, scales, rots, upstream_batch, accumulate=False,
                                         upstream_view=upstream_view)
                flat.all_reduce()
            return images
        flat.zero_()
        if batch is not None:       # the same through autograd, view by view
            images = batch.run(views_of(s), rasterize, lambda v, img: dL)
        else:
            images = []
            for v in views_of(s):
                img = rasterize(v)[0]
                img.backward(dL)
                images.append(img.detach())
        flat.all_reduce()
        return images

    # the first batch renders its views synchronously and learns the instance bound that sizes the sync-free steps' buffers (SyncFreeBatch)
    step(0)
    torch.cuda.synchronize()
    prof_all, kern, dom = {}, {}, None
    if a.full:
        # per-stage times FIRST: one untimed pass with events around every stage (each event costs queue time, so the timed region below keeps
        # only the events of the dominant kernel -- the one the roofline object reports) on ONE stream.  Until round 5 this pass stood between the
        # warm-up and the timed blocks, and the first block was the slow one in every line (1.86-1.89 ms against 1.72-1.74 for the other two: the
        # stream pools of the caching allocator and the speculation state had last seen the one-stream pass) -- a second hiccup in one of the other
        # two blocks then made that block the median (one line in six: 892 Gfrag/s between 946 and 979).  Now the W warm-up steps run directly in
        # front of the K timed ones, in the configuration that is timed.
        _C.profile_begin(max(a.warmup, 2) * VPG * 8 + 64)
        if batch is not None:
            batch.streams = 1                                    # one stream: every kernel has the GPU to itself
        for s in range(max(a.warmup, 2)):
            step(s)
        torch.cuda.synchronize()
        if batch is not None:
            batch.streams = a.streams
        prof_all = _C.profile_end()
        kern = {k: (ms / max(n, 1)) for k, (ms, n) in prof_all.items() if n > 0}
        dom = max(kern, key=lambda k: prof_all[k][0]) if kern else None          # most time per step (a batched kernel runs once per step)
    # The interpreter's full garbage collection walks every object torch and the scene set-up have created -- ~65 ms on the round's boxes, at a
    # step count the allocation counters decide (tools/trainer_protocol.py <deg> 20 8: one 60-70 ms step per ~150, none with the collector off),
    # i.e. 3 ms per step of whichever block it falls into.  Collect now and move what is alive to the permanent generation: the collector stays
    # ON for everything the steps allocate.  In FRONT of the warm-up: the collection is a host-side gap of that length, and the GPU should come
    # to the timed blocks from the warm-up steps, not from idling.
    gc.collect()
    gc.freeze()
    for s in range(a.warmup):
        step(s)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    # The timed region carries NO instrumentation: a HIP event around a kernel is a barrier packet in its queue, and the two events per launch
    # of the dominant kernel that round 1 kept here cost ~15 us per launch (rocprof trace: gaps of that size in front of every k_render_bwd).
    # EXACTLY a.steps steps are timed, in three consecutive blocks (one when there are fewer than six), each bracketed by a barrier + device
    # synchronisation on both sides; per block the MAX over ranks, and the headline is the MEDIAN block's time per step (box-to-box and
    # block-to-block spread of a 40-ms region is 1-2 %: one block was the whole headline until round 3).  `elapsed_total` keeps the sum.
    n_blocks_t = 3 if a.steps >= 6 else 1
    bounds = [a.steps * i // n_blocks_t for i in range(n_blocks_t + 1)]
    block_s = []

    for bi in range(n_blocks_t):
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(bounds[bi], bounds[bi + 1]):
            images = step(s)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        block_s.append(time.perf_counter() - t0)
    if a.dump_outputs and rank == 0:            # before anything else runs a step: the images are a buffer the next step reuses
        dump_outputs(a.dump_outputs, images, {n: t.grad for n, t in zip(("means3D", "opacities", "scales", "rotations", "shs"), params)},
                     batch.viewspace_grads if (batch is not None and not a.per_view_calls) else None)
    # the dominant kernel as it runs when the streams share the GPU: the same steps again, now with events around that kernel only
    dom_timed = None
    if dom:
        _C.profile_begin(min(a.steps, 10) * VPG + 64, stages=[dom])
        for s in range(min(a.steps, 10)):
            step(s)
        torch.cuda.synchronize()
        prof = _C.profile_end()
        dom_timed = prof[dom][0] / prof[dom][1] if prof[dom][1] > 0 else None

    F_rank = sum(F_view[v] for s in range(a.steps) for v in views_of(s))
    R_rank = sum(R_view[v] for s in range(a.steps) for v in views_of(s))
    frames_rank = a.steps * VPG
    if dist is not None:
        t = torch.tensor(block_s, device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        block_s = [float(x) for x in t.tolist()]
        c = torch.tensor([F_rank, R_rank], device=dev, dtype=torch.int64)
        dist.all_reduce(c)
        F_tot, R_tot = int(c[0].item()), int(c[1].item())
    else:
        F_tot, R_tot = F_rank, R_rank
    block_ms_per_step = [block_s[bi] / max(bounds[bi + 1] - bounds[bi], 1) * 1e3 for bi in range(n_blocks_t)]
    elapsed_total = sum(block_s)
    elapsed = sorted(block_ms_per_step)[n_blocks_t // 2] * 1e-3 * a.steps          # a.steps steps at the median block's rate

    if rank == 0:
        ms_per_step = elapsed / a.steps * 1e3
        value = F_tot / elapsed / 1e6
        # dominant kernel and its roofline (algorithmic bytes per launch: DESIGN.md "Roofline accounting")
        Rm = R_rank / frames_rank
        Npix = W * H
        Cin = 12 * (D + 1) ** 2 if a.mode == "sh" else 12
        alg = {   # bytes per launch, single-touch model (SURVEY.md section 8d terms, regrouped per kernel)
            "preprocess_fwd": (44 + Cin + (75 if a.mode == "sh" else 60)) * P + 4 * Rm,
            "scan": 8 * P / 256 + 12 * (Npix / 256),
            "scatter": 20 * P + 12 * Rm,
            "tile_sort": (8 + 8 + 36 + 40 + 4) * Rm,
            "render_fwd": 40 * Rm + 20 * Npix,
            "render_bwd": 44 * Rm + 20 * Npix + 36 * Rm,
            "preprocess_bwd": (36 * Rm) + ((107 + Cin) + (40 + Cin) + 56 + 36) * P if a.mode == "sh" else (36 * Rm) + (92 + 40 + 56 + 36) * P,
        }
        if batch is not None and batch.deferred:   # one launch for the VPG views of the step: shared rows once, per-view state VPG times
            alg["preprocess_bwd"] = VPG * (36 * Rm + (24 + 1 + 4 + 4 + 4 + 12) * P) + (40 + Cin + 2 * (44 + Cin)) * P
        roof = None
        if dom:
            # Dominant kernel = most time per step.  Its duration is measured LIVE with HIP events on the launch stream, in the one-stream pass
            # above where the kernel has the GPU to itself (in the timed region up to `streams` launches share the GPU and stretch each other:
            # avg_launch_ms_streams_sharing_the_gpu).  The roofline object is priced against HBM (the path's bounding roofline):
            # achieved = algorithmic bytes of the launch / that duration.  For the render kernels, which sit far below it because they are bound
            # by vector-instruction issue and LDS, the object carries `valu_issue` as the explanation: wave-instructions
            # per launch (a PMC count of the same workload committed under profiles/) / duration against the chip's issue peak.  Counter figures
            # are quoted only when the committed set was collected on the SAME kernel sources (csrc_sha16): otherwise traffic is null.
            prof_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
            traffic, valu_insts, counters_note = None, None, None
            if a.config in (3, 4) and a.mode == "sh":
                try:
                    from youreditableavatar_amd.build import source_hash
                    pmc = json.load(open(os.path.join(prof_dir, PROFILE_SET + "_hbm_counters.json")))
                    sq = json.load(open(os.path.join(prof_dir, PROFILE_SET + "_sq_counters.json")))
                    if pmc.get("csrc_sha16") == source_hash() == sq.get("csrc_sha16"):
                        traffic = next(v["hbm_bytes_est"] for k, v in pmc["kernels"].items() if k.startswith("tgs::k_" + dom))
                        valu_insts = next(v["SQ_INSTS_VALU"] for k, v in sq["kernels"].items() if k.startswith("tgs::k_" + dom))
                        counters_note = PROFILE_SET + "_{hbm,sq}_counters.json (same kernel sources: csrc_sha16 " + pmc["csrc_sha16"] + ")"
                    else:
                        counters_note = (f"profiles/{PROFILE_SET}_*_counters.json were collected on other kernel sources (csrc_sha16 {pmc.get('csrc_sha16')} vs "
                                         f"{source_hash()}): not quoted")
                except (OSError, StopIteration, KeyError, ValueError):
                    pass
            Rb = sum(Rb_view[v] for s in range(a.steps) for v in views_of(s)) / frames_rank     # instances the timed path really bins
            # `achieved` / `frac` (round 5, ADVICE): SURVEY.md 8d's per-unit bytes x the units THIS launch processes -- for k_render_bwd 40 B per
            # instance the kernel walks (the binned ones: instance pruning leaves out a fifth of the reference's) + 20 N (pixels in) + 44 P (the
            # per-Gaussian sums it produces).  Beside it the same with the reference's instance count (`frac_reference_instances`: what rounds 3-4
            # quoted as `frac`; it counts bytes this kernel never moves) and `bytes_own_layout`: what this library's layout really moves for the
            # launch (48-B records + quadrant mask + slot in, one 48-B slab row per binned instance out).
            alg_8d = dict(alg)
            alg_8d["render_bwd"] = 40 * Rb + 20 * Npix + 44 * P
            alg_8d["render_fwd"] = 40 * Rb + 20 * Npix
            a8_ref = {"render_bwd": 40 * Rm + 20 * Npix + 44 * P, "render_fwd": 40 * Rm + 20 * Npix}.get(dom, alg[dom])
            alg_b = dict(alg)
            alg_b["render_fwd"] = 48 * Rb + 20 * Npix
            alg_b["render_bwd"] = (48 + 4 + 48) * Rb + 20 * Npix          # records + quadrant mask + slot in, one 48-B slab row out; pixels in
            t_alone = kern[dom]
            a8, ab = alg_8d.get(dom, alg[dom]), alg_b.get(dom, alg[dom])
            roof = {"kernel": "k_" + dom, "bound": "hbm", "achieved": round(a8 / (t_alone * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(a8 / (t_alone * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "traffic": traffic,
                    "algorithmic_bytes_per_launch": int(a8), "bytes_model": "SURVEY.md 8d per-unit bytes x the units this launch processes (its binned instances, pixels, Gaussians)",
                    "frac_reference_instances": round(a8_ref / (t_alone * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "bytes_own_layout": int(ab), "frac_own_layout": round(ab / (t_alone * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "instances_reference": int(Rm), "instances": int(Rb),
                    "avg_launch_ms": round(t_alone, 4), "duration": "kernel alone on the GPU (one-stream pass of this run, HIP events on the launch stream)",
                    "avg_launch_ms_streams_sharing_the_gpu": round(dom_timed, 4) if dom_timed else None, "concurrent_streams": batch.streams if batch is not None else 1,
                    "counters": counters_note}
            if dom in ("render_fwd", "render_bwd") and valu_insts:
                ach = valu_insts / (t_alone * 1e-3) / 1e9
                roof["valu_issue"] = {"what": "the bound that applies to this kernel: vector-instruction issue (+ the LDS accumulator), DESIGN.md section 6",
                                      "achieved": round(ach, 1), "peak": VALU_PEAK_GWIPS, "unit": "G wave-instr/s", "frac": round(ach / VALU_PEAK_GWIPS, 4),
                                      "valu_instructions_per_launch": int(valu_insts), "peak_measured_v_fma_f32": VALU_MEASURED_FMA_GWIPS,
                                      "peak_measured_render_mix": VALU_MEASURED_MIX_GWIPS, "frac_of_measured_render_mix": round(ach / VALU_MEASURED_MIX_GWIPS, 4)}
        k_P = (430 + 3 * Cin) if a.mode == "sh" else 412
        B_alg = k_P * P + 124 * Rm + 40 * Npix
        per_view = alg["scan"] + alg["scatter"] + alg["tile_sort"] + alg["render_fwd"] + alg["render_bwd"]
        pre_out = (75 if a.mode == "sh" else 60) * P + 4 * Rm
        pair = batch is not None and not a.per_view_calls
        B_step = (VPG / 2 if pair else VPG) * (44 + Cin) * P + VPG * pre_out + VPG * per_view + (alg["preprocess_bwd"] if (batch is not None and batch.deferred) else VPG * alg["preprocess_bwd"])
        out = {
            "metric": "rasterized fragments/sec (fwd+bwd) @500k Gaussians 1080p" if a.config in (3, 4) else f"rasterized fragments/sec (fwd+bwd) config {a.config}",
            "value": round(value, 2), "unit": "Mfrag/s", "n_gpus": N, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "timing": {"blocks": n_blocks_t, "steps_per_block": [bounds[i + 1] - bounds[i] for i in range(n_blocks_t)], "ms_per_step_blocks": [round(x, 4) for x in block_ms_per_step],
                       "headline": "median block", "ms_per_step_all_blocks": round(elapsed_total / a.steps * 1e3, 4)},
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"cfg{a.config}: {P} Gaussians, {W}x{H}, SH degree {D}, colour mode {a.mode}, {V}-view orbit, {VPG} frames per GPU per step",
                       "frames_per_step": N * VPG, "views_per_gpu_per_step": VPG, "fragments_per_frame": int(F_rank / frames_rank),
                       "instances_per_frame": int(Rm), "instances_binned_per_frame": int(sum(Rb_view[v] for s in range(a.steps) for v in views_of(s)) / frames_rank) if Rb_view else None, "ms_per_frame_per_gpu": round(ms_per_step / VPG, 4),
                       "host_sync": "one per step (SyncFreeBatch)" if batch is not None else "one per frame (reference protocol)",
                       "upstream": "fused L1+SSIM loss against target images (tgs_l1_ssim)" if a.loss else "fixed dL/d image",
                       "native_calls": ("3 per step (run_views)" if not a.per_view_calls else "per view, through autograd") if batch is not None else "per view",
                       "streams": batch.streams if batch is not None else 1,
                       "per_gaussian_backward": "one pass per step (tgs_backward_batch)" if (batch is not None and batch.deferred) else "one pass per view",
                       "frames_rerendered": batch.rejected if batch is not None else 0,
                       "sync_free_grid_tiles": (batch.tile_capacity() if batch is not None else 0) or None,   # bound on the tiles with instances the sync-free grids are sized for (learned from the previous steps; None: all tiles)
                       "parallelism": f"view-sharded dp{N}: {N} rank(s) x 1 GPU, torch.distributed world size {dist.get_world_size() if dist is not None else 1} "
                                      f"(backend {a.backend if N > 1 else 'none'}), {n_devices} GPU(s) visible per node"
                                      + ((f", gradient all-reduce in {chunks} Gaussian ranges overlapped with the per-Gaussian pass" if (chunks > 1 and batch is not None and not a.per_view_calls)
                                          else ", one all-reduce of the flat gradient buffer per step") if N > 1 else "")},
            "roofline": roof,
            "kernels_ms": {k: round(v, 4) for k, v in kern.items()},      # each kernel alone on the GPU (one-stream pass before the timed region)
            "frame_algorithmic_bytes": int(B_alg),
            # single-touch bytes of ONE step of the batch path: what the headline's timed region has to move -- the SH rows once per PAIR of views
            # (k_preprocess_fwd_pair), the per-Gaussian backward ONCE per step (its shared rows once, per-view state VPG times)
            "batch_step_algorithmic_bytes": int(B_step),
            "batch_step_hbm_frac": round(B_step / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
            "hbm_frac_of_8TBps": {"batch_step": round(B_step / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "dominant_kernel": roof["frac"] if roof else None,
                                  "what": "algorithmic bytes / time / 8 TB/s: one step of the batch path with ITS OWN single-touch bytes (timed region), the dominant kernel "
                                          "alone on the GPU with SURVEY.md 8d's bytes; the single frame through the drop-in API: secondary.dropin_api.frame_hbm_frac"},
            "other_rates": {"Minstances/s": round(R_tot / elapsed / 1e6, 2), "Mpixels/s": round(Npix * frames_rank * N / elapsed / 1e6, 2),
                            "MGaussians/s": round(P * frames_rank * N / elapsed / 1e6, 2), "frames/s": round(frames_rank * N / elapsed, 1)},
        }
        if a.full and N == 1 and not a.no_secondary and a.mode == "sh" and batch is not None and not a.per_view_calls:
            del batch                                        # (its pooled state: ~2 GB)
            torch.cuda.empty_cache()
            out["secondary"] = secondary_workloads(a, cloud, dev, D, W, H, out["config"]["ms_per_frame_per_gpu"])
            out["config"]["dropin_ms_per_frame"] = out["secondary"]["dropin_api"]["ms_per_frame"]
            # the honest single-frame figure: SURVEY.md 8d's B_alg over the frame time of the path the reference's trainers call
            out["secondary"]["dropin_api"]["frame_hbm_frac"] = round(B_alg / (out["secondary"]["dropin_api"]["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
            out["dropin_frame_hbm_frac"] = out["secondary"]["dropin_api"]["frame_hbm_frac"]
        if a.full and N == 1 and not a.no_cpu:
            out["cpu_baseline"] = cpu_baseline(cloud, cams[0], dL_np, a)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def dump_outputs(out_dir, images, grads, viewspace):
    """--dump-outputs: what the last timed step handed its caller -- the rendered images, the parameter gradients and (whole-batch path) dL/d means2D
    per view -- as float32 ``<name>.npy`` files, so that two builds can be compared output for output.  An array over its budget is a sample at
    fixed seeded positions: the same pixels of every view and channel, the same Gaussians of every per-Gaussian array (at most 56 MB in all)."""
    if isinstance(images, (list, tuple)):
        images = torch.stack(images)
    V, _, H, W = images.shape
    grads = {n: g for n, g in grads.items() if g is not None}
    P = next(iter(grads.values())).shape[0]

    def pick(n, k, seed):
        idx = np.arange(n) if n <= k else np.sort(np.random.default_rng(seed).choice(n, k, replace=False))
        return torch.from_numpy(idx).to(images.device)

    pixels = pick(H * W, (6 << 20) // (V * 3), 1)                                # <= 24 MB of images
    # room for dL/d means2D whether or not the path returns it: every path of the same workload samples the same Gaussians
    per_gaussian = sum(g[0].numel() for g in grads.values()) + V * 3
    rows = pick(P, (8 << 20) // per_gaussian, 2)                                 # <= 32 MB of per-Gaussian arrays
    arrays = {"images": images.reshape(V, 3, H * W)[:, :, pixels]}
    arrays.update({"grad_" + n: g[rows] for n, g in grads.items()})
    if viewspace is not None:
        arrays["grad_means2D"] = viewspace[:, rows]
    os.makedirs(out_dir, exist_ok=True)
    for n, t in arrays.items():
        np.save(os.path.join(out_dir, n + ".npy"), t.detach().float().cpu().numpy())


def secondary_workloads(a, cloud, dev, D, W, H, headline_ms):
    """Reported beside the headline, never as it (N = 1, outside the timed region, a few seconds in all):

    * ``dropin_api``: one view per step through the UNCHANGED reference API -- ``GaussianRasterizer(settings)(...)`` + ``image.backward(dL)``, SH
      colours evaluated in the rasterizer, one read-back of num_rendered per frame taken off the critical path (tgs_forward_speculative) --
      what a caller that swaps the package and changes nothing else gets per frame (the headline is the 8-view batch API).
    * ``trainer_protocol``: what the reference's trainers run per optimisation step (tetgs_texture/paint_2dgs.py:159-166, refine_3dgs.py:165-166,
      tetgs_scene/tetgs_model.py:524-537,605-614, refine.py:245-247): 2048 x 2048, colours from SH OUTSIDE the rasterizer (sh_color.points_rgb,
      ``colors_precomp``), the L1 + SSIM loss between forward and backward, one random view per step, everything through autograd.
    * ``grown_splats``: the headline batch path with every splat 4x / 8x larger (most splats on 5..64 tiles).
    * ``alive_pairs``: (pixel, list entry) pairs of view 0 with alpha >= 1/255 -- what the render kernels actually blend; the fragment metric
      F = sum n_contrib also counts the entries a pixel walks past."""
    import math
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.loss import l1_ssim_loss
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
    from youreditableavatar_amd.sh_color import points_rgb_dc_rest
    from youreditableavatar_amd.bindings import gaussian_bind
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    P = cloud["means3D"].shape[0]
    g = lambda x, rg=False: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).requires_grad_(rg)

    def settings_for(w, h, deg, n):
        out = []
        for k in range(n):
            c = scenes.orbit_camera(w, h, azimuth_deg=(k * 137.5) % 360.0)          # golden-angle sequence: consecutive views far apart, like a shuffled camera list
            out.append(GaussianRasterizationSettings(image_height=h, image_width=w, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg), scale_modifier=1.0,
                                                     viewmatrix=g(c.viewmatrix), projmatrix=g(c.projmatrix), sh_degree=deg, campos=g(c.campos), prefiltered=False,
                                                     debug=False))
        return out

    def timed(fn, n, warm, blocks=3):
        # median of `blocks` timed blocks of n calls: a block that happens to contain an allocator miss (the per-frame state buffers of the
        # drop-in path are fresh torch tensors sized by the frame's instance count) reported 0.48 instead of 0.38 ms per frame now and then
        gc.collect()
        gc.freeze()                                         # (see the headline's timed region: a full collection inside a 20-call block is 3 ms per call;
        for i in range(warm):                               #  in front of the warm-up, so that the GPU comes to the first block from work, not from idling)
            fn(i)
        out = []
        for b in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                fn(warm + b * n + i)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / n * 1e3)
        return sorted(out)[len(out) // 2]

    res = {}
    leaves = {k: g(cloud[k], True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    # ---- the unchanged drop-in API, one view per step
    S = settings_for(W, H, D, 16)
    dL = g(scenes.upstream_gradient(W, H, seed=4321))

    def dropin(i):
        for t in leaves.values():
            t.grad = None                                   # optimizer.zero_grad(set_to_none=True), as the reference's trainers do every step (refine.py:323)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        img, _radii = GaussianRasterizer(S[i % len(S)])(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                                                        scales=leaves["scales"], rotations=leaves["rotations"])
        img.backward(dL)
    res["dropin_api"] = {"ms_per_frame": round(timed(dropin, 40, 20), 4), "what": f"GaussianRasterizer + autograd, one view per step, {W}x{H}, SH degree {D} in the rasterizer",
                         "vs_headline_batch_path": round(timed(dropin, 20, 0, 1) / headline_ms, 2)}
    # Host share of the same loop ON THIS BOX (round 5): the wall time per frame beside (a) the GPU's own span of the loop -- HIP events behind the
    # first launch and the last completion on the loop's stream -- and (b) the sum of the library's stage times of an instrumented pass (tgs_profile_*:
    # events around every stage; the caller's own kernels -- the zero fill of means2D -- are not in it).  wall - gpu_span is time the GPU waited for the host.
    try:
        n = 40
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        dropin(0)
        e0.record()                                         # (behind the first frame: the GPU is busy from here on if the host keeps up)
        for i in range(1, n + 1):
            dropin(i)
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / (n + 1) * 1e3
        span = e0.elapsed_time(e1) / n
        _C.profile_begin(64 * n)
        for i in range(n):
            dropin(i)
        torch.cuda.synchronize()
        pr = _C.profile_end()
        ksum = sum(ms for ms, c in pr.values() if c) / n
        res["dropin_api"].update({"gpu_span_ms_per_frame": round(span, 4), "wall_ms_per_frame_same_loop": round(wall, 4),
                                  "host_share_ms_per_frame": round(max(wall - span, 0.0), 4), "library_stage_sum_ms_per_frame": round(ksum, 4),
                                  "stages_ms": {k: round(ms / max(c, 1) , 4) for k, (ms, c) in pr.items() if c}})
    except Exception as ex:                                 # noqa: BLE001 -- a secondary measurement must not take the line down
        res["dropin_api"]["host_share_error"] = repr(ex)[:200]
    # ---- the trainers' protocol at 2048 x 2048
    TW = TH = 2048
    gt = torch.rand(3, TH, TW, device=dev)
    tp = {}
    # the model's own colour parameters (tetgs_model.py:234-239): _sh_coordinates_dc [P,1,3] and, for models with more than one level,
    # _sh_coordinates_rest [P,15,3]; the inpainting-stage models have one level and no rest tensor
    sh_dc = g(cloud["shs"][:, :1], True)
    sh_rest = g(cloud["shs"][:, 1:], True)
    # ... and its raw geometry parameters (tetgs_model.py:196-229): densities before the sigmoid, log-scales, unnormalised quaternions
    op_np = np.clip(cloud["opacities"], 1e-4, 1 - 1e-4)
    raw = {"all_densities": g(np.log(op_np / (1 - op_np)), True), "_scales": g(np.log(cloud["scales"]), True), "_quaternions": g(cloud["rotations"], True)}
    for deg in (0, 3):
        S2 = settings_for(TW, TH, deg, 16)
        colour_params = [sh_dc] + ([sh_rest] if deg > 0 else [])

        def train_step(i, S2=S2, deg=deg, colour_params=colour_params):
            rs = S2[i % len(S2)]
            for t in [leaves["means3D"]] + list(raw.values()) + colour_params:
                t.grad = None
            colors = points_rgb_dc_rest(sh_dc, sh_rest if deg > 0 else None, deg + 1, positions=leaves["means3D"], camera_centers=rs.campos)
            opacities, scales_a, rotations_a, _ = gaussian_bind(raw["all_densities"], raw["_scales"], raw["_quaternions"])   # strengths / scaling / quaternions
            m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
            img, _radii = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=opacities, colors_precomp=colors,
                                                 scales=scales_a, rotations=rotations_a)
            l1_ssim_loss(img, gt, 0.2).backward()
        tp[f"sh{deg}"] = round(timed(train_step, 20, 10), 4)
    res["trainer_protocol"] = {"ms_per_step": tp, "what": f"{P} Gaussians, 2048x2048, one view per step from the model's RAW parameters: bindings.gaussian_bind (sigmoid / exp / normalize, "
                               "one kernel) + sh_color.points_rgb_dc_rest (dc / rest parameters, no torch.cat) -> GaussianRasterizer(colors_precomp) -> l1_ssim_loss -> backward, all through autograd (SH degree 0: the inpainting stage, "
                               "a one-level model, 16 800 of the reference's ~22 800 rasterizer iterations; 3: refinement)"}
    del gt
    # ---- grown splats through the headline path
    gs = {}
    for mult in (4.0, 8.0):
        big = {k: (g(cloud[k] * (mult if k == "scales" else 1.0), True)) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
        FlatGradients([big[k] for k in ("means3D", "opacities", "scales", "rotations", "shs")])
        b2 = SyncFreeBatch(streams=a.streams)
        S3 = settings_for(W, H, D, 8)
        ms = timed(lambda i: b2.run_views(S3, big["means3D"], big["opacities"], big["shs"], big["scales"], big["rotations"], None, accumulate=False,
                                          upstream_view=lambda v, image: dL), 6, 3) / len(S3)
        gs[f"x{int(mult)}"] = {"ms_per_frame": round(ms, 4), "frames_rerendered": b2.rejected}
        try:
            # per stage, each kernel alone on the GPU (one stream, events around every stage) -- and the SAME cloud one view per step through the unchanged
            # GaussianRasterizer API with its single-frame fraction of the HBM peak (round 6: large splats are the regime the reference trains in,
            # tetgs_edit_2d.py:203; the 2.5 tiles per splat of config 3 are the synthetic floor)
            b2.streams = 1
            b2.run_views(S3, big["means3D"], big["opacities"], big["shs"], big["scales"], big["rotations"], None, accumulate=False, upstream_view=lambda v, image: dL)
            torch.cuda.synchronize()
            _C.profile_begin(64 * len(S3))
            b2.run_views(S3, big["means3D"], big["opacities"], big["shs"], big["scales"], big["rotations"], None, accumulate=False, upstream_view=lambda v, image: dL)
            torch.cuda.synchronize()
            pr = _C.profile_end()
            gs[f"x{int(mult)}"]["stages_ms_per_frame_alone"] = {k: round(ms_ / len(S3), 4) for k, (ms_, c) in pr.items() if c}
            counts = []

            def dropin_big(i):
                for t in big.values():
                    t.grad = None
                m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
                img, _ = GaussianRasterizer(S3[i % len(S3)])(means3D=big["means3D"], means2D=m2, opacities=big["opacities"], shs=big["shs"], scales=big["scales"], rotations=big["rotations"])
                img.backward(dL)
            ms1 = timed(dropin_big, 8, 6)
            rs_ = S3[0]
            e_ = torch.Tensor([])
            Rb = int(_C.rasterize_gaussians(rs_.bg, big["means3D"].detach(), e_, big["opacities"].detach(), big["scales"].detach(), big["rotations"].detach(), 1.0, e_, rs_.viewmatrix,
                                            rs_.projmatrix, rs_.tanfovx, rs_.tanfovy, H, W, big["shs"].detach(), D, rs_.campos, False, False)[0])
            Cin_ = 12 * (D + 1) ** 2
            B_ = (430 + 3 * Cin_) * P + 124 * Rb + 40 * W * H
            gs[f"x{int(mult)}"].update({"dropin_ms_per_frame": round(ms1, 4), "instances_binned_view0": Rb, "frame_algorithmic_bytes": int(B_),
                                        "frame_hbm_frac": round(B_ / (ms1 * 1e-3) / 1e9 / 8000.0, 5)})
        except Exception as ex:                             # noqa: BLE001 -- a secondary measurement must not take the line down
            gs[f"x{int(mult)}"]["breakdown_error"] = repr(ex)[:200]
        del b2, big
        torch.cuda.empty_cache()
    gs["what"] = ("every splat x 4 / x 8 (most on 5..64 tiles): ms_per_frame in 8-view batches (the headline path), stages_ms_per_frame_alone from a one-stream pass with events "
                  "around every stage, dropin_ms_per_frame one view per step through GaussianRasterizer; frame_hbm_frac = SURVEY 8d's bytes with THIS frame's binned instances / drop-in time / 8 TB/s")
    res["grown_splats"] = gs
    # ---- the same cloud with its Gaussians numbered along a Morton curve (mesh-bound Gaussians come spatially ordered; the generator's order is random)
    mc = scenes.morton_order(cloud)
    co = {k: g(mc[k], True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    FlatGradients([co[k] for k in ("means3D", "opacities", "scales", "rotations", "shs")])
    b3 = SyncFreeBatch(streams=a.streams)
    S4 = settings_for(W, H, D, 8)
    ms = timed(lambda i: b3.run_views(S4, co["means3D"], co["opacities"], co["shs"], co["scales"], co["rotations"], None, accumulate=False,
                                      upstream_view=lambda v, image: dL), 10, 4) / len(S4)
    res["spatially_ordered_gaussians"] = {"ms_per_frame": round(ms, 4), "what": "the headline path on the same cloud re-numbered along a 3-D Morton curve (index neighbours share tiles: the "
                                          "gathers hit neighbouring lines; the binning has no global atomics, so the order no longer decides its cost)"}
    del b3, co
    torch.cuda.empty_cache()
    try:
        # ... and with every splat x 4 on top: spatially ordered AND on 5..64 tiles is what a mesh-bound trained scene looks like (tetgs_edit_2d.py:203)
        co = {k: g(mc[k] * (4.0 if k == "scales" else 1.0), True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
        FlatGradients([co[k] for k in ("means3D", "opacities", "scales", "rotations", "shs")])
        b4 = SyncFreeBatch(streams=a.streams)
        ms4 = timed(lambda i: b4.run_views(S4, co["means3D"], co["opacities"], co["shs"], co["scales"], co["rotations"], None, accumulate=False,
                                           upstream_view=lambda v, image: dL), 6, 3) / len(S4)
        res["spatially_ordered_gaussians"]["x4_ms_per_frame"] = round(ms4, 4)
        del b4, co
    except Exception as ex:                                 # noqa: BLE001 -- a secondary measurement must not take the line down
        res["spatially_ordered_gaussians"]["x4_error"] = repr(ex)[:200]
    torch.cuda.empty_cache()
    # ---- alive (pixel, entry) pairs of view 0
    rs = S[0]
    e = torch.Tensor([])
    R, _c, _r, geom, binning, img = _C.rasterize_gaussians(rs.bg, leaves["means3D"].detach(), e, leaves["opacities"].detach(), leaves["scales"].detach(),
                                                          leaves["rotations"].detach(), 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W,
                                                          leaves["shs"].detach(), D, rs.campos, False, False)
    f = lambda n: _C.state_field(n, P, W, H, R, True, True, geom, binning, img)
    pl, rg, m2, co = f("point_list").long(), f("ranges").view(-1, 2).long(), f("means2D").view(-1, 2), f("conic_opacity").view(-1, 4)
    gx = (W + 15) // 16
    tile_of = torch.repeat_interleave(torch.arange(rg.shape[0], device=dev), rg[:, 1] - rg[:, 0])
    px = torch.arange(16, device=dev, dtype=torch.float32)
    alive_pairs = 0
    for s0 in range(0, R, 1 << 18):
        ids, t = pl[s0:s0 + (1 << 18)], tile_of[s0:s0 + (1 << 18)]
        dx = m2[ids, 0, None, None] - (((t % gx) * 16).float()[:, None, None] + px[None, None, :])
        dy = m2[ids, 1, None, None] - (((t // gx) * 16).float()[:, None, None] + px[None, :, None])
        q = co[ids]
        power = -0.5 * (q[:, 0, None, None] * dx * dx + q[:, 2, None, None] * dy * dy) - q[:, 1, None, None] * dx * dy
        alive_pairs += int(((power <= 0) & (torch.clamp(q[:, 3, None, None] * torch.exp(power), max=0.99) >= 1.0 / 255.0)).sum())
    # ---- the N > 1 step's collective path through the REAL backend (RCCL) at world size 1: tools/rccl_world1.py as a CHILD process with a time
    # limit, started after this process has released its big allocations -- a problem in the collective library must not take the line down
    try:
        import subprocess
        torch.cuda.empty_cache()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_world1.py"), str(a.config)], capture_output=True, text=True, timeout=240)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        res["rccl_world1"] = json.loads(line[-1]) if (r.returncode == 0 and line) else {"error": f"rc {r.returncode}: " + (r.stderr or "")[-300:]}
    except Exception as ex:          # noqa: BLE001 (TimeoutExpired included)
        res["rccl_world1"] = {"error": repr(ex)[:300]}
    res["alive_pairs"] = {"per_frame_view0": alive_pairs, "G_pairs_per_s_at_headline_rate": round(alive_pairs / (headline_ms * 1e-3) / 1e9, 2),
                          "what": "(pixel, tile-list entry) pairs with alpha >= 1/255 (forward.cu:340-343) of view 0, termination ignored"}
    return res


def cpu_baseline(cloud, cam, dL_np, a):
    """The CPU oracle (C restatement of the reference, OpenMP over tiles) timed on this box's host
    cores on the SAME workload frame (view 0): a reported baseline, not the target.  Beside it, BASELINE.json's named baseline: the
    PyTorch-autograd point-splat (oracle/torch_splat.py, float32) on BASELINE config 1 (10k Gaussians, 256 x 256, SH degree 0)."""
    from oracle import oracle
    mode = a.mode
    t_all = []
    F = 0
    for i in range(a.cpu_frames):
        t0 = time.perf_counter()
        color, radii, st, grads = oracle.run_scene(cloud, cam, dL_np, mode=mode)
        t_all.append(time.perf_counter() - t0)
        F = int(st.field("n_contrib").astype(np.int64).sum())
        del st
    t = float(np.median(t_all))
    out = {"value": round(F / t / 1e6, 2), "unit": "Mfrag/s", "cores": oracle.threads(), "kind": "port",
           "sample": f"{a.cpu_frames} full fwd+bwd frames of view 0 of the same workload (median {t:.2f} s/frame, F={F})",
           "host_cpus": os.cpu_count()}
    # north_star's named baseline as a CHILD process with a time limit: thousands of small tensor operations whose speed on a 128-thread host
    # is not this benchmark's to guarantee -- the leg must not hold the line up (round 3: with all host threads it did, for minutes)
    try:
        import subprocess
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-splat-only"], capture_output=True, text=True, timeout=150)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        out["torch_point_splat_cfg1"] = json.loads(line[-1]) if (r.returncode == 0 and line) else {"error": f"rc {r.returncode}: " + (r.stderr or "")[-200:]}
    except Exception as ex:          # noqa: BLE001 -- a baseline leg must not take the bench line down (TimeoutExpired included)
        out["torch_point_splat_cfg1"] = {"error": repr(ex)[:200]}
    return out


def torch_point_splat_cfg1(frames: int = 6):
    """north_star's CPU baseline as named: "the reference's CPU fallback (PyTorch autograd point-splat) timed on the host cores" on BASELINE
    config 1 -- 10 000 random Gaussians, 256 x 256, SH degree 0, white background, one orbit camera, upstream N(0,1)/(3HW) (BASELINE.md
    section 3).  oracle/torch_splat.py in float32 on 16 host threads: forward + autograd backward, median of up to `frames` frames
    after one warm-up (at most ~25 s).  F = sum of n_contrib of that frame."""
    import torch as th
    from oracle import torch_splat
    from youreditableavatar_amd import scenes
    cfg = scenes.CONFIGS[1]
    cloud = scenes.config_cloud(1)
    cam = scenes.orbit_camera(cfg["width"], cfg["height"])
    dL1 = scenes.upstream_gradient(cfg["width"], cfg["height"], seed=cfg["seed"] + 1000)
    old = th.get_num_threads()
    # per-tile tensors of a few hundred kB: intra-op threading beyond a NUMA node's worth of cores only adds synchronisation (with all 128
    # threads of the GPU box's host the leg ran for minutes); 16 threads, stated in `cores`
    th.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        ts, F = [], 0
        t_start = time.perf_counter()
        for i in range(frames + 1):
            t0 = time.perf_counter()
            r = torch_splat.run_scene(cloud, cam, dL1, mode="sh", dtype=th.float32)
            if i > 0:
                ts.append(time.perf_counter() - t0)
            F = int(r["n_contrib"].sum())
            if i > 0 and time.perf_counter() - t_start > 25.0:         # bounded sample (~10-30 s of CPU work)
                break
        frames = len(ts)
        t = float(np.median(ts))
        return {"value": round(F / t / 1e6, 3), "unit": "Mfrag/s", "cores": th.get_num_threads(), "kind": "port (PyTorch autograd point-splat, float32)",
                "sample": f"{frames} fwd+bwd frames of BASELINE config 1 (10k Gaussians, 256x256, SH0), median {t * 1e3:.0f} ms/frame, F={F}",
                "ms_per_frame": round(t * 1e3, 1)}
    finally:
        th.set_num_threads(old)


if __name__ == "__main__":
    main()
