#!/usr/bin/env python3
"""Picking the Gaussians under a 2-D mask, and fitting positions to a target median-depth map, with the rasterizer's median outputs
(``GaussianRasterizer(...)(..., return_median=True)``: median_depth[1,H,W] and median_index[1,H,W] -- view-space z and Gaussian index of
the first blended splat after which the transmittance falls below one half; 0 and -1 where it never does):

  1. a synthetic cloud  ->  one view  ->  ``median_index[mask]`` of a rectangle mask = the Gaussians that ARE the visible surface under it
     (with a mesh-bound model ``tetgs._face_indices[...]`` of those is the set of faces under the mask); prints how many were picked;
  2. the cloud pushed away from the camera  ->  loss = l1_loss(median_depth, target) against the original cloud's map  ->  autograd  ->
     FusedAdam on the positions.  median_depth is piecewise constant in every alpha: its gradient reaches the positions alone, so the
     positions are the only thing fitted here (a loss on the EXPECTED depth, return_depth=True, is the one that moves opacities).

Asserts that something was picked and that the loss falls; prints it at steps 0 and N.
Usage:  python examples/pick_and_fit_median.py [--steps 40] [--gaussians 5000] [--size 160 120]
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
    from youreditableavatar_amd.optim import FusedAdam
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
        _color, _radii, median_depth, median_index = rasterizer(means3D=p["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True),
                                                                opacities=p["opacities"], shs=p["shs"], scales=p["scales"], rotations=p["rotations"],
                                                                return_median=True)
        return median_depth, median_index

    with torch.no_grad():
        target, index = (x.clone() for x in render(truth))
    # 1. a 2-D mask lifted to the Gaussians under it: the middle third of the image
    mask = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
    mask[:, H // 3:2 * H // 3, W // 3:2 * W // 3] = True
    under = index[mask]
    picked = torch.unique(under[under >= 0])                # (-1: the transmittance stays at or above one half -- no surface at that pixel)
    n_picked = int(picked.numel())
    log(f"picked {n_picked} of {P} Gaussians under a {W // 3} x {H // 3} mask ({int((under >= 0).sum())} of its {int(mask.sum())} pixels have a surface)")
    assert n_picked > 0, "no Gaussian under the mask"
    # 2. positions fitted to the median-depth map
    params = {k: v.clone() for k, v in truth.items()}
    params["means3D"] = (params["means3D"] + 0.25 * view_dir.reshape(1, 3)).contiguous().requires_grad_(True)      # what the optimiser has to undo
    opt = FusedAdam([{"params": [params["means3D"]], "lr": 1e-2}])
    losses = []
    for step in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        median_depth, _ = render(params)
        loss = l1_loss(median_depth, target)
        loss.backward()
        losses.append(loss.detach())                        # (a device tensor: no host sync inside the step)
        if step < steps:
            opt.step()
    vals = [float(x) for x in losses]
    log(f"step {0:3d}  loss {vals[0]:.5f}")
    log(f"step {steps:3d}  loss {vals[-1]:.5f}")
    assert vals[-1] < vals[0], "the loss did not fall"
    return n_picked, vals


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--size", type=int, nargs=2, default=[160, 120])
    a = ap.parse_args()
    run(a.steps, a.gaussians, a.size[0], a.size[1])
