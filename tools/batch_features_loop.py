"""What feature channels cost in the whole-batch path: config 3's cloud, 8 views per step through SyncFreeBatch.run_views(upstream_batch), in the modes
  plain:          no features (today's step);
  features4:      features=F[P,4] and an upstream gradient on the feature map (tgs_features_views: k_feat_fwd; k_feat_bwd per view behind
                  the colour's backward; k_feat_bwd_gauss_views once per step);
  features16:     the same at C = 16 (two channel groups per view each way);
  workaround4 / workaround16:
                  what a step had to do without it: the plain step, then ceil(C / 3) further run_views steps with colors_precomp = F[:, triple]
                  per view and background 0, whose images are the map's triples and whose colour gradients are dL/dF -- each repeating
                  preprocess, binning, sort and the per-Gaussian backward;
alternating in blocks on one device -- `python3 tools/batch_features_loop.py [steps per block] [rounds] [W H]` (default: config 3's 1920 x 1080), or
under `rocprofv3 --kernel-trace --stats -- python3 tools/batch_features_loop.py ...` for the kernels' own times.  Step times are host-clock times
around blocks that end in a device synchronise; every mode is warmed up on every shape it uses before the first timed block.  Prints ms per step
and per frame for every mode.  On a tree whose run_views has no ``features`` only `plain` and the workarounds run: the same loop on the parent
commit is the yardstick for "features cost nothing when absent" -- plain must be within the spread of its own blocks there."""
import inspect, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
from youreditableavatar_amd import scenes
from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
from diff_gaussian_rasterization import GaussianRasterizationSettings
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
rng = np.random.Generator(np.random.PCG64(4325))
CS = (4, 16)
F = {C: g(rng.standard_normal((P, C)).astype(np.float32), True) for C in CS}
for C in CS:
    F[C].grad = torch.zeros_like(F[C])
dF = {C: g((rng.standard_normal((V, C, H, W)) / (H * W)).astype(np.float32)) for C in CS}


def settings(bg):
    out = []
    for k in range(16):
        c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
        out.append(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg if bg is None else bg), scale_modifier=1.0,
                                                 viewmatrix=g(c.viewmatrix), projmatrix=g(c.projmatrix), sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False))
    return out


S, S0 = settings(None), settings(np.zeros(3, np.float32))
dL = g(scenes.upstream_gradient(W, H, seed=4321))
has_features = "features" in inspect.signature(SyncFreeBatch.run_views).parameters
MODES = ("plain",) + (tuple(f"features{C}" for C in CS) if has_features else ()) + tuple(f"workaround{C}" for C in CS)
# the workaround's inputs: the triples of F as per-view colours (the same for every view) and of the upstream as colour gradients, zero-padded
triples = lambda C: [list(range(c, min(c + 3, C))) for c in range(0, C, 3)]
WCOL, WDL = {}, {}
for C in CS:
    for cols in triples(C):
        col = torch.zeros((P, 3), device=dev); col[:, :len(cols)] = F[C].detach()[:, cols]
        d = torch.zeros((V, 3, H, W), device=dev); d[:, :len(cols)] = dF[C][:, cols]
        WCOL[C, cols[0]], WDL[C, cols[0]] = col[None].expand(V, P, 3).contiguous(), d
# one object (bound, pooled buffers) per mode and kind of step: a mode never pays for another's pool
batch = {m: SyncFreeBatch() for m in MODES}
wbatch = {C: SyncFreeBatch() for C in CS}


def step(i, mode):
    views = [S[(i + k) % len(S)] for k in range(V)]
    args = (L["means3D"], L["opacities"], L["shs"], L["scales"], L["rotations"])
    if mode.startswith("features"):
        C = int(mode[len("features"):])
        batch[mode].run_views(views, *args, lambda images, fmap: (dL, dF[C]), accumulate=False, features=F[C])
        return
    batch[mode].run_views(views, *args, lambda images: dL, accumulate=False)
    if mode.startswith("workaround"):
        C = int(mode[len("workaround"):])
        views0 = [S0[(i + k) % len(S0)] for k in range(V)]
        for cols in triples(C):                             # the through-alpha share is added to the parameters' gradients, dL/dF is color_grads summed over the views
            wbatch[C].run_views(views0, L["means3D"], L["opacities"], None, L["scales"], L["rotations"], lambda images, c0=cols[0]: WDL[C, c0], accumulate=True,
                                colors_precomp=WCOL[C, cols[0]])
            F[C].grad[:, cols] = wbatch[C].color_grads.sum(0)[:, :len(cols)]


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
res = {"size": [W, H], "views_per_step": V, "steps_per_block": steps, "modes": list(MODES),
       "rejected": {**{m: batch[m].rejected for m in MODES}, **{f"workaround{C}_extra": wbatch[C].rejected for C in CS}}}
for m in MODES:
    res[m + "_ms_per_step"], res[m + "_mean"], res[m + "_ms_per_frame"] = ms[m], mean(ms[m]), round(mean(ms[m]) / V, 4)
res["plain_spread"] = round(max(ms["plain"]) - min(ms["plain"]), 4)
for m in MODES[1:]:
    res[m + "_adds_per_frame"] = round((res[m + "_mean"] - res["plain_mean"]) / V, 4)
print(json.dumps(res))
