"""What the expected-depth output costs, and what it replaces: tools/dropin_loop.py's step (one view per step through GaussianRasterizer + autograd,
config 3's cloud) next to
  depth:     the same step with return_depth=True and an upstream gradient on depth as well (one frame, three more kernels);
  two_frame: the workaround without the output -- the plain step plus a SECOND frame of the same geometry with colors_precomp = z.expand(-1, 3),
             bg = 0, z computed in torch from means3D (so that its gradient reaches the positions), its channel 0 taking the depth's upstream;
the three alternating in blocks on one device -- `python3 tools/depth_loop.py [steps per block] [rounds] [W H]` (default: config 3's 1920 x 1080;
`2048 2048` for the trainers' size), or under `rocprofv3 --kernel-trace --stats -- python3 tools/depth_loop.py ...` for the times of k_depth_fwd,
k_depth_bwd and k_depth_bwd_gauss.  The claim to read off: (depth - plain) < (two_frame - plain) by more than the spread of the plain blocks."""
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
S, S0, ZROW = [], [], []
for k in range(16):
    c = scenes.orbit_camera(W, H, azimuth_deg=(k * 137.5) % 360.0)
    kw = dict(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, scale_modifier=1.0, viewmatrix=g(c.viewmatrix), projmatrix=g(c.projmatrix),
              sh_degree=D, campos=g(c.campos), prefiltered=False, debug=False)
    S.append(GaussianRasterizationSettings(bg=g(c.bg), **kw))
    S0.append(GaussianRasterizationSettings(bg=g(np.zeros(3, np.float32)), **kw))
    m = np.asarray(c.viewmatrix, np.float32).reshape(-1)
    ZROW.append((g(m[[2, 6, 10]].reshape(3, 1)), float(m[14])))
dL = g(scenes.upstream_gradient(W, H, seed=4321))
dD = g((np.random.Generator(np.random.PCG64(4323)).standard_normal((1, H, W)) / (H * W)).astype(np.float32))
dD3 = torch.cat([dD, torch.zeros(2, H, W, device=dev)], 0)
MODES = ("plain", "depth", "two_frame")


def step(i, mode):
    for t in L.values():
        t.grad = None                                       # optimizer.zero_grad(set_to_none=True) (refine.py:323)
    v = i % len(S)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    out = GaussianRasterizer(S[v])(means3D=L["means3D"], means2D=m2, opacities=L["opacities"], shs=L["shs"], scales=L["scales"], rotations=L["rotations"],
                                   return_depth=mode == "depth")
    if mode == "depth":
        torch.autograd.backward([out[0], out[2]], [dL, dD])
        return
    out[0].backward(dL)
    if mode == "two_frame":
        row, off = ZROW[v]
        z = L["means3D"] @ row + off
        m2b = torch.zeros(P, 3, device=dev, requires_grad=True)
        frame = GaussianRasterizer(S0[v])(means3D=L["means3D"], means2D=m2b, opacities=L["opacities"], colors_precomp=z.expand(-1, 3), scales=L["scales"],
                                          rotations=L["rotations"])
        frame[0].backward(dD3)


for i in range(21):
    step(i, MODES[i % 3])
ms = {m: [] for m in MODES}
for r in range(rounds):
    for mode in MODES:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(21 + r * steps + i, mode)
        torch.cuda.synchronize()
        ms[mode].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
mean = lambda v: round(sum(v) / max(len(v), 1), 4)
res = {"size": [W, H], "steps_per_block": steps}
for m in MODES:
    res[m + "_ms_per_frame"], res[m + "_mean"] = ms[m], mean(ms[m])
res["plain_spread"] = round(max(ms["plain"]) - min(ms["plain"]), 4)
res["depth_adds"], res["two_frame_adds"] = round(res["depth_mean"] - res["plain_mean"], 4), round(res["two_frame_mean"] - res["plain_mean"], 4)
print(json.dumps(res))
