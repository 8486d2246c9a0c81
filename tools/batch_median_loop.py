"""What the median costs behind the whole-batch step: config 3's cloud, 8 views per step through SyncFreeBatch.run_views(upstream_batch), in the modes
  plain:          the step alone (today's step);
  median:         the step, then median_views() (k_median_fwd per view on the lanes);
  median+grad:    the step, median_views(), then backward_median_views(dL) (k_median_bwd per view, k_depth_bwd_gauss_views once per step);
  median+votes:   the step, median_views(), then surface_votes over the V index maps with a rectangle mask (k_surface_votes);
alternating in blocks on one device -- `python3 tools/batch_median_loop.py [steps per block] [rounds] [W H]` (default: config 3's 1920 x 1080), or under
`rocprofv3 --kernel-trace --stats -- python3 tools/batch_median_loop.py ...` for the kernels' own times.  Prints ms per step and per frame for every
mode.  On a tree whose SyncFreeBatch has no median_views, or with an older library (TGS_LIBRARY), only `plain`
runs: the same loop on the parent commit is the yardstick for "run_views without the new calls did not slow down" -- plain must be within the spread of its own blocks there.
(k_surface_votes issues one atomic per run of equal indices in a wave; a one-atomic-per-pixel kernel to compare it with does not exist in this
tree, so no such pair of figures is printed.)"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
from youreditableavatar_amd import multiview, scenes
from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
from diff_gaussian_rasterization import GaussianRasterizationSettings, _C
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
V = 8
dev = torch.device("cuda", 0)
cfg = scenes.CONFIGS[3]; P, W, H, D = cfg["P"], cfg["width"], cfg["height"], cfg["sh_degree"]
if len(sys.argv) > 4:
    W, H = int(sys.argv[3]), int(sys.argv[4])
cloud = scenes.config_cloud(3)
g = lambda x, rg=False: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).requires_grad_(rg)
names = ("means3D", "opacities", "scales", "rotations", "shs")
L = {k: g(cloud[k], True) for k in names}
flat = FlatGradients([L[k] for k in names])
S = []
for k in range(16):
    c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
    S.append(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg), scale_modifier=1.0, viewmatrix=g(c.viewmatrix),
                                           projmatrix=g(c.projmatrix), sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False))
dL = g(scenes.upstream_gradient(W, H, seed=4321))
rng = np.random.Generator(np.random.PCG64(4324))
dM = g((rng.standard_normal((V, 1, H, W)) / (H * W)).astype(np.float32))
masks = torch.zeros((V, 1, H, W), dtype=torch.bool, device=dev)
masks[:, :, H // 3:2 * H // 3, W // 3:2 * W // 3] = True
seen, hits = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
has_median = hasattr(SyncFreeBatch, "median_views") and hasattr(_C._lib, "tgs_median_views")      # (TGS_LIBRARY: an older build of the library)
MODES = ("plain", "median", "median+grad", "median+votes") if has_median else ("plain",)
batch = {m: SyncFreeBatch() for m in MODES}                 # one object (bound, pooled buffers) per mode: a mode never pays for another's pool


def step(i, mode):
    views = [S[(i + k) % len(S)] for k in range(V)]
    b = batch[mode]
    b.run_views(views, L["means3D"], L["opacities"], L["shs"], L["scales"], L["rotations"], lambda images: dL, accumulate=False)
    if mode != "plain":
        _depth, index = b.median_views()
        if mode == "median+grad":
            b.backward_median_views(dM)
        elif mode == "median+votes":
            multiview.surface_votes(index, P, masks, out=(seen, hits))


for i in range(6 * len(MODES)):
    step(i, MODES[i % len(MODES)])
ms = {m: [] for m in MODES}
for r in range(rounds):
    for mode in MODES:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(r * steps + i, mode)
        torch.cuda.synchronize()
        ms[mode].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
mean = lambda v: round(sum(v) / max(len(v), 1), 4)
res = {"size": [W, H], "views_per_step": V, "steps_per_block": steps, "modes": list(MODES), "rejected": {m: batch[m].rejected for m in MODES}}
for m in MODES:
    res[m + "_ms_per_step"], res[m + "_mean"], res[m + "_ms_per_frame"] = ms[m], mean(ms[m]), round(mean(ms[m]) / V, 4)
res["plain_spread"] = round(max(ms["plain"]) - min(ms["plain"]), 4)
for m in MODES[1:]:
    res[m + "_adds_per_frame"] = round((res[m + "_mean"] - res["plain_mean"]) / V, 4)
print(json.dumps(res))
