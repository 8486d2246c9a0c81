"""What the accumulated-alpha output costs: tools/dropin_loop.py's step (one view per step through GaussianRasterizer + autograd, config 3's cloud)
next to the same step with return_alpha=True and an upstream gradient on alpha as well, the two alternating in blocks on one device --
`python3 tools/alpha_loop.py [steps per block] [rounds] [W H]` (default: config 3's 1920 x 1080; `2048 2048` for the trainers' size), or under
`rocprofv3 --kernel-trace --stats -- python3 tools/alpha_loop.py ...` for the times of k_alpha and of the per-pixel backward with and without the
alpha gradient.  TGS_DETERMINISTIC=1 times the fixed-order kernels instead."""
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
S = []
for k in range(16):
    c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
    S.append(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=g(c.bg), scale_modifier=1.0, viewmatrix=g(c.viewmatrix),
                                           projmatrix=g(c.projmatrix), sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False))
dL = g(scenes.upstream_gradient(W, H, seed=4321))
dA = g((np.random.Generator(np.random.PCG64(4322)).standard_normal((1, H, W)) / (H * W)).astype(np.float32))


def step(i, with_alpha):
    for t in L.values():
        t.grad = None                                       # optimizer.zero_grad(set_to_none=True) (refine.py:323)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    out = GaussianRasterizer(S[i % len(S)])(means3D=L["means3D"], means2D=m2, opacities=L["opacities"], shs=L["shs"], scales=L["scales"], rotations=L["rotations"],
                                            return_alpha=with_alpha)
    if with_alpha:
        torch.autograd.backward([out[0], out[2]], [dL, dA])
    else:
        out[0].backward(dL)


for i in range(20):
    step(i, i % 2 == 1)
ms = {False: [], True: []}
for r in range(rounds):
    for with_alpha in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(20 + r * steps + i, with_alpha)
        torch.cuda.synchronize()
        ms[with_alpha].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
mean = lambda v: round(sum(v) / max(len(v), 1), 4)
print(json.dumps({"size": [W, H], "steps_per_block": steps, "plain_ms_per_frame": ms[False], "alpha_ms_per_frame": ms[True],
                  "plain_mean": mean(ms[False]), "alpha_mean": mean(ms[True])}))
