#!/usr/bin/env python3
"""Fitting a cloud's opacities, scales and positions to target masks and depth maps of several views per step, on the whole-batch path
(``SyncFreeBatch.run_views(..., return_alpha=True, return_depth=True)``: three trips into the library per step, nothing read back per frame):

  a cloud pushed outwards, shrunken and faded  ->  alpha[V,1,H,W] and depth[V,1,H,W] of V orbit views in one batch
  ->  loss = l1(alpha, masks) + l1(depth / alpha, target depths) against the original cloud's maps, evaluated by ``upstream_batch`` on the
  maps (autograd on two small tensors; the images take no part: their gradient is zero)  ->  the batch's backward adds every view's
  gradients into the parameters' ``.grad``  ->  FusedAdam.

The multi-view sibling of fit_silhouette.py and fit_depth.py.  Asserts that the loss falls; prints it at steps 0 and N.
Usage:  python examples/fit_views_silhouette_depth.py [--steps 60] [--gaussians 5000] [--size 160 120] [--views 6]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(steps=60, P=5000, W=160, H=120, views=6, seed=0, device="cuda", log=print):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch
    from youreditableavatar_amd.optim import FusedAdam
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    cloud = scenes.make_cloud(P, 1, seed=seed, scale_mult=3.0)
    names = ("means3D", "opacities", "scales", "rotations", "shs")
    truth = {k: t(cloud[k]) for k in names}
    settings = []
    for k in range(views):
        c = scenes.orbit_camera(W, H, azimuth_deg=360.0 * k / views, bg=(0.0, 0.0, 0.0))
        settings.append(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
            projmatrix=t(c.projmatrix), sh_degree=int(cloud["sh_degree"]), campos=t(c.campos), prefiltered=False, debug=False))
    no_colour = torch.zeros(3, H, W, device=dev)            # dL/d images, the same for every view: the images take no part in the loss
    normalised = lambda alpha, depth: depth / alpha.clamp_min(1e-3)

    def batch_of(p):
        leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
        return leaves, FlatGradients([leaves[k] for k in names]), SyncFreeBatch()

    def step_of(leaves, batch, upstream):
        return batch.run_views(settings, leaves["means3D"], leaves["opacities"], leaves["shs"], leaves["scales"], leaves["rotations"], upstream,
                               accumulate=False, return_alpha=True, return_depth=True)

    # targets: coverage masks and normalised depths of the original cloud, from the same path (zero gradients: nothing is fitted here)
    leaves, _flat, batch = batch_of(truth)
    _images, alpha, depth = step_of(leaves, batch, lambda images, a, d: (no_colour, None, None))
    masks, targets = alpha.clone(), normalised(alpha, depth).clone()

    start = dict(truth)
    start["means3D"] = truth["means3D"] * 1.15                                # what the optimiser has to undo: pushed outwards ...
    start["scales"] = truth["scales"] * 0.7                                   # ... shrunken ...
    start["opacities"] = (truth["opacities"] * 0.5).clamp(0.02, 0.99)         # ... and faded
    leaves, _flat, batch = batch_of(start)
    opt = FusedAdam([{"params": [leaves["means3D"]], "lr": 4e-3}, {"params": [leaves["opacities"]], "lr": 2e-2}, {"params": [leaves["scales"]], "lr": 2e-3}])
    losses = []

    def upstream(images, alpha, depth):
        a, d = alpha.detach().requires_grad_(True), depth.detach().requires_grad_(True)
        loss = (a - masks).abs().mean() + (normalised(a, d) - targets).abs().mean()
        g_alpha, g_depth = torch.autograd.grad(loss, (a, d))
        losses.append(loss.detach())                        # (a device tensor: no host sync inside the step)
        return no_colour, g_alpha, g_depth

    for step in range(steps + 1):
        del losses[step:]                                   # (a batch that renders a view again calls upstream twice: keep the last)
        step_of(leaves, batch, upstream)
        losses[step:] = losses[-1:]
        if step < steps:
            opt.step()
            with torch.no_grad():
                leaves["opacities"].clamp_(0.01, 0.99)
                leaves["scales"].clamp_(min=1e-4)
    vals = [float(x) for x in losses]
    log(f"step {0:3d}  loss {vals[0]:.5f}")
    log(f"step {steps:3d}  loss {vals[-1]:.5f}")
    assert vals[-1] < vals[0], "the loss did not fall"
    return vals


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--size", type=int, nargs=2, default=[160, 120])
    ap.add_argument("--views", type=int, default=6)
    a = ap.parse_args()
    run(a.steps, a.gaussians, a.size[0], a.size[1], a.views)
