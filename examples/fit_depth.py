#!/usr/bin/env python3
"""Fitting a cloud's positions and opacities to a target depth map with the rasterizer's expected-depth output
(``GaussianRasterizer(...)(..., return_alpha=True, return_depth=True)``: depth[1,H,W] = sum_i T_i alpha_i z_i, differentiable):

  a cloud pushed away from the camera and faded  ->  alpha and depth of one view through the drop-in API
  ->  loss = l1_loss(depth / alpha, target depth) + l1_loss(alpha, target coverage) against the original cloud's maps  ->  autograd  ->  Adam.

The normalised depth is the caller's expression: both of its terms are outputs of ONE frame, and one backward call carries both upstream
gradients (the image takes no part in the loss).  Asserts that the loss falls; prints it at steps 0 and N.
Usage:  python examples/fit_depth.py [--steps 40] [--gaussians 5000] [--size 160 120]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(steps=40, P=5000, W=160, H=120, seed=0, device="cuda", log=print):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.loss import l1_loss
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    cloud = scenes.make_cloud(P, 1, seed=seed, scale_mult=3.0)
    truth = {k: t(cloud[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    c = scenes.orbit_camera(W, H, azimuth_deg=20.0, bg=(0.0, 0.0, 0.0))
    rasterizer = GaussianRasterizer(GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
        projmatrix=t(c.projmatrix), sh_degree=int(cloud["sh_degree"]), campos=t(c.campos), prefiltered=False, debug=False))
    view_dir = t(np.asarray(c.viewmatrix, np.float32).reshape(-1)[[2, 6, 10]])      # d z / d mean: the third row of the view transform

    def render(p):
        _color, _radii, alpha, depth = rasterizer(means3D=p["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True), opacities=p["opacities"],
                                                  shs=p["shs"], scales=p["scales"], rotations=p["rotations"], return_alpha=True, return_depth=True)
        return alpha, depth / alpha.clamp_min(1e-3)

    with torch.no_grad():                                   # targets: coverage and normalised depth of the original cloud
        cover, target = (x.clone() for x in render(truth))
    params = {k: v.clone() for k, v in truth.items()}
    params["means3D"] = params["means3D"] + 0.25 * view_dir.reshape(1, 3)    # what the optimiser has to undo: pushed back ...
    params["opacities"] = (params["opacities"] * 0.6).clamp(0.02, 0.99)      # ... and faded
    fitted = [params["means3D"].requires_grad_(True), params["opacities"].requires_grad_(True)]
    opt = torch.optim.Adam([{"params": [fitted[0]], "lr": 1e-2}, {"params": [fitted[1]], "lr": 2e-2}])
    losses = []
    for step in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        alpha, depth = render(params)
        loss = l1_loss(depth, target) + l1_loss(alpha, cover)
        loss.backward()
        losses.append(loss.detach())                        # (a device tensor: no host sync inside the step)
        if step < steps:
            opt.step()
            with torch.no_grad():
                fitted[1].clamp_(0.01, 0.99)
    vals = [float(x) for x in losses]
    log(f"step {0:3d}  loss {vals[0]:.5f}")
    log(f"step {steps:3d}  loss {vals[-1]:.5f}")
    assert vals[-1] < vals[0], "the loss did not fall"
    return vals


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--size", type=int, nargs=2, default=[160, 120])
    a = ap.parse_args()
    run(a.steps, a.gaussians, a.size[0], a.size[1])
