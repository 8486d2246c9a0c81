"""What the feature-channel output costs, and what it replaces: tools/dropin_loop.py's step (one view per step through GaussianRasterizer + autograd,
config 3's cloud) next to
  feat4 / feat16:  the same step with features=F[P,C] (C = 4, 16) and an upstream gradient on the feature map as well (one frame; one or two
                   launches of k_feat_fwd / k_feat_bwd and k_feat_bwd_gauss more);
  work4 / work16:  the workaround without the output -- the plain step plus ceil(C / 3) further frames of the same geometry with
                   colors_precomp = F[:, 3k:3k+3] (zero-padded), bg = 0, each taking its triple of the map's upstream;
the five alternating in blocks on one device -- `python3 tools/feature_loop.py [steps per block] [rounds] [W H]` (default: config 3's 1920 x 1080),
or under `rocprofv3 --kernel-trace --stats -- python3 tools/feature_loop.py ...` for the times of k_feat_fwd, k_feat_bwd and k_feat_bwd_gauss.
The claim to read off: (featC - plain) < (workC - plain) at both channel counts, by more than the spread of the plain blocks."""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
from youreditableavatar_amd import scenes
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
cfg = scenes.CONFIGS[3]; P, W, H, D = cfg["P"], cfg["width"], cfg["height"], cfg["sh_degree"]
if len(sys.argv) > 4:
    W, H = int(sys.argv[3]), int(sys.argv[4])
cloud = scenes.config_cloud(3)
g = lambda x, rg=False: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).requires_grad_(rg)
L = {k: g(cloud[k], True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
S, S0 = [], []
for k in range(16):
    c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
    kw = dict(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, scale_modifier=1.0, viewmatrix=g(c.viewmatrix), projmatrix=g(c.projmatrix),
              sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False)
    S.append(GaussianRasterizationSettings(bg=g(c.bg), **kw))
    S0.append(GaussianRasterizationSettings(bg=g(np.zeros(3, np.float32)), **kw))
dL = g(scenes.upstream_gradient(W, H, seed=4321))
rng = np.random.Generator(np.random.PCG64(4324))
CH = (4, 16)
F = {C: g(rng.standard_normal((P, C)), True) for C in CH}
dF = {C: g((rng.standard_normal((C, H, W)) / (H * W)).astype(np.float32)) for C in CH}
# the workaround's upstream per triple, zero-padded to three channels
dF3 = {C: [torch.cat([dF[C][k:k + 3], torch.zeros(3 - min(3, C - k), H, W, device=dev)], 0) for k in range(0, C, 3)] for C in CH}
MODES = ("plain", "feat4", "work4", "feat16", "work16")


def step(i, mode):
    for t in list(L.values()) + list(F.values()):
        t.grad = None                                       # optimizer.zero_grad(set_to_none=True) (refine.py:323)
    v = i % len(S)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    C = int(mode[4:]) if mode != "plain" else 0
    out = GaussianRasterizer(S[v])(means3D=L["means3D"], means2D=m2, opacities=L["opacities"], shs=L["shs"], scales=L["scales"], rotations=L["rotations"],
                                   features=F[C] if mode.startswith("feat") else None)
    if mode.startswith("feat"):
        torch.autograd.backward([out[0], out[2]], [dL, dF[C]])
        return
    out[0].backward(dL)
    if mode.startswith("work"):
        for n, k in enumerate(range(0, C, 3)):
            cols = F[C][:, k:k + 3]
            if cols.shape[1] < 3:
                cols = torch.cat([cols, torch.zeros(P, 3 - cols.shape[1], device=dev)], 1)
            m2b = torch.zeros(P, 3, device=dev, requires_grad=True)
            frame = GaussianRasterizer(S0[v])(means3D=L["means3D"], means2D=m2b, opacities=L["opacities"], colors_precomp=cols, scales=L["scales"],
                                              rotations=L["rotations"])
            frame[0].backward(dF3[C][n])


for i in range(20):
    step(i, MODES[i % len(MODES)])
ms = {m: [] for m in MODES}
for r in range(rounds):
    for mode in MODES:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(20 + r * steps + i, mode)
        torch.cuda.synchronize()
        ms[mode].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
mean = lambda v: round(sum(v) / max(len(v), 1), 4)
res = {"size": [W, H], "steps_per_block": steps}
for m in MODES:
    res[m + "_ms_per_frame"], res[m + "_mean"] = ms[m], mean(ms[m])
res["plain_spread"] = round(max(ms["plain"]) - min(ms["plain"]), 4)
for C in CH:
    res[f"feat{C}_adds"], res[f"work{C}_adds"] = round(res[f"feat{C}_mean"] - res["plain_mean"], 4), round(res[f"work{C}_mean"] - res["plain_mean"], 4)
print(json.dumps(res))
