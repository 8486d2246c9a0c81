#!/usr/bin/env python3
"""Fitting a cloud's per-Gaussian features and opacities to target feature maps of several views per step, on the whole-batch path
(``SyncFreeBatch.run_views(..., features=F)``: three trips into the library per step, nothing read back per frame):

  features F[P,4] -- three signed channels (a normal-like vector) and one mask channel -- started from noise, opacities faded
  ->  feature_map[V,4,H,W] of V orbit views in one batch
  ->  loss = l1(feature_map, targets) against the maps of the original cloud with its true features, evaluated by ``upstream_batch`` on the
  map (autograd on one small tensor; the images take no part: their gradient is zero)  ->  the batch's backward stores dL/dF of all views in
  ``F.grad`` and adds the through-alpha share of every view into the opacities' ``.grad``  ->  FusedAdam on both.

The multi-view sibling of fit_features.py, modelled on fit_views_silhouette_depth.py.  Asserts that the loss falls; prints it at steps 0 and N.
Usage:  python examples/fit_views_features.py [--steps 60] [--gaussians 5000] [--size 160 120] [--views 6]
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
    # the true features: the direction of the Gaussian from the cloud's centre (signed, unit length) and a mask of the upper half
    centred = truth["means3D"] - truth["means3D"].mean(0, keepdim=True)
    true_F = torch.cat([centred / centred.norm(dim=1, keepdim=True).clamp_min(1e-6), (centred[:, 1:2] > 0).float()], dim=1).contiguous()
    settings = []
    for k in range(views):
        c = scenes.orbit_camera(W, H, azimuth_deg=360.0 * k / views, bg=(0.0, 0.0, 0.0))
        settings.append(GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
            projmatrix=t(c.projmatrix), sh_degree=int(cloud["sh_degree"]), campos=t(c.campos), prefiltered=False, debug=False))
    no_colour = torch.zeros(3, H, W, device=dev)            # dL/d images, the same for every view: the images take no part in the loss

    def batch_of(p, F):
        leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
        leaves["features"] = F.detach().clone().requires_grad_(True)
        return leaves, FlatGradients([leaves[k] for k in names + ("features",)]), SyncFreeBatch()

    def step_of(leaves, batch, upstream):
        return batch.run_views(settings, leaves["means3D"], leaves["opacities"], leaves["shs"], leaves["scales"], leaves["rotations"], upstream,
                               accumulate=False, features=leaves["features"])

    # targets: the feature maps of the original cloud with its true features, from the same path (no gradient: nothing is fitted here)
    leaves, _flat, batch = batch_of(truth, true_F)
    _images, fmap = step_of(leaves, batch, lambda images, m: (no_colour, None))
    targets = fmap.clone()

    gen = torch.Generator(device=dev).manual_seed(seed)
    start = dict(truth)
    start["opacities"] = (truth["opacities"] * 0.5).clamp(0.02, 0.99)         # what the optimiser has to undo: faded ...
    leaves, _flat, batch = batch_of(start, 0.1 * torch.randn(true_F.shape, device=dev, generator=gen))      # ... and features that know nothing
    opt = FusedAdam([{"params": [leaves["features"]], "lr": 5e-2}, {"params": [leaves["opacities"]], "lr": 1e-2}])
    losses = []

    def upstream(images, fmap):
        m = fmap.detach().requires_grad_(True)
        loss = (m - targets).abs().mean()
        (g,) = torch.autograd.grad(loss, (m,))
        losses.append(loss.detach())                        # (a device tensor: no host sync inside the step)
        return no_colour, g

    for step in range(steps + 1):
        del losses[step:]                                   # (a batch that renders a view again calls upstream twice: keep the last)
        step_of(leaves, batch, upstream)
        losses[step:] = losses[-1:]
        if step < steps:
            opt.step()
            with torch.no_grad():
                leaves["opacities"].clamp_(0.01, 0.99)
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
