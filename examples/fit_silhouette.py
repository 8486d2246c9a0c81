#!/usr/bin/env python3
"""Fitting a cloud's opacities and scales to a target silhouette with the rasterizer's accumulated-alpha output
(``GaussianRasterizer(...)(..., return_alpha=True)``: alpha[1,H,W] = 1 - final_T, differentiable):

  a cloud with shrunken, faded splats  ->  colour and alpha of a few orbit views through the drop-in API
  ->  loss = l1_loss(color, gt) + l1_loss(alpha, mask) against the original cloud's images and coverage  ->  autograd  ->  Adam.

One backward call per view carries both upstream gradients.  Prints the loss at steps 0 and N.
Usage:  python examples/fit_silhouette.py [--steps 40] [--gaussians 5000] [--size 160 120] [--views 4]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(steps=40, P=5000, W=160, H=120, V=4, seed=0, device="cuda", log=print):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.loss import l1_loss
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    cloud = scenes.make_cloud(P, 1, seed=seed, scale_mult=3.0)
    truth = {k: t(cloud[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    rasterizers = []
    for k in range(V):
        c = scenes.orbit_camera(W, H, azimuth_deg=360.0 * k / V, bg=(0.0, 0.0, 0.0))
        rasterizers.append(GaussianRasterizer(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
            projmatrix=t(c.projmatrix), sh_degree=int(cloud["sh_degree"]), campos=t(c.campos), prefiltered=False, debug=False)))

    def render(r, p):
        color, _radii, alpha = r(means3D=p["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True), opacities=p["opacities"], shs=p["shs"],
                                 scales=p["scales"], rotations=p["rotations"], return_alpha=True)
        return color, alpha

    with torch.no_grad():                                   # targets: images and coverage masks of the original cloud
        targets = [tuple(x.clone() for x in render(r, truth)) for r in rasterizers]
    params = {k: v.clone() for k, v in truth.items()}
    params["opacities"] = (params["opacities"] * 0.4).clamp(0.02, 0.99)      # what the optimiser has to undo: faded ...
    params["scales"] = params["scales"] * 0.6                                # ... and shrunken splats
    fitted = [params["opacities"].requires_grad_(True), params["scales"].requires_grad_(True)]
    opt = torch.optim.Adam([{"params": [fitted[0]], "lr": 2e-2}, {"params": [fitted[1]], "lr": 2e-3}])
    losses = []
    for step in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for r, (gt, mask) in zip(rasterizers, targets):
            color, alpha = render(r, params)
            loss = l1_loss(color, gt) + l1_loss(alpha, mask)
            loss.backward()
            total = total + loss.detach()
        losses.append(total / V)                            # (a device tensor: no host sync inside the step)
        if step < steps:
            opt.step()
            with torch.no_grad():
                fitted[0].clamp_(0.01, 0.99)
                fitted[1].clamp_(min=1e-4)
    vals = [float(x) for x in losses]
    log(f"step {0:3d}  loss {vals[0]:.5f}")
    log(f"step {steps:3d}  loss {vals[-1]:.5f}")
    return vals


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--size", type=int, nargs=2, default=[160, 120])
    ap.add_argument("--views", type=int, default=4)
    a = ap.parse_args()
    run(a.steps, a.gaussians, a.size[0], a.size[1], a.views)
