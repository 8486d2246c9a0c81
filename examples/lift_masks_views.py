#!/usr/bin/env python3
"""Lifting 2-D edit masks of several views to the Gaussians, and fitting positions to target median-depth maps of all views per step, on the
whole-batch path (``SyncFreeBatch.run_views`` with ``median_views()`` / ``backward_median_views(dL)`` behind it; nothing read back per frame):

  1. a synthetic cloud  ->  V orbit views in one batch  ->  ``median_index[V,1,H,W]``  ->  ``surface_votes(median_index, P, masks)`` with a
     rectangle mask per view = per Gaussian, over all views, the pixels where it IS the visible surface (seen) and how many of them lie
     inside the masks (hits); ``hits / seen`` above one half picks the Gaussians under the masks (with a mesh-bound model
     ``tetgs._face_indices[picked]`` is the set of faces to edit: the reference's back_project / hit_tri_id_Set, from splats instead of rays);
  2. the cloud pushed away from its centre  ->  loss = mean |median_depth - target| over all views against the original cloud's maps  ->
     ``backward_median_views`` adds every view's share into ``means3D.grad``  ->  FusedAdam on the positions.  median_depth is piecewise
     constant in every alpha: its gradient reaches the positions alone (the images take no part in the loss: their gradient is zero).

Asserts that something was picked and that the loss falls; prints the pick and the loss at steps 0 and N.
Usage:  python examples/lift_masks_views.py [--steps 40] [--gaussians 5000] [--size 160 120] [--views 6]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(steps=40, P=5000, W=160, H=120, views=6, seed=0, device="cuda", log=print):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.multiview import FlatGradients, SyncFreeBatch, surface_votes
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

    def batch_of(p):
        leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
        return leaves, FlatGradients([leaves[k] for k in names]), SyncFreeBatch()

    def step_of(leaves, batch):
        batch.run_views(settings, leaves["means3D"], leaves["opacities"], leaves["shs"], leaves["scales"], leaves["rotations"], lambda images: no_colour,
                        accumulate=False)
        return batch.median_views()

    # 1. the masks lifted to the Gaussians: the middle third of every view
    leaves, _flat, batch = batch_of(truth)
    target, index = (x.clone() for x in step_of(leaves, batch))
    masks = torch.zeros((views, 1, H, W), dtype=torch.bool, device=dev)
    masks[:, :, H // 3:2 * H // 3, W // 3:2 * W // 3] = True
    seen, hits = surface_votes(index, P, masks)
    picked = (seen > 0) & (2 * hits > seen)                 # hits / seen > 1/2, in integers; a boolean per Gaussian, still on the device
    n_seen, n_picked = int((seen > 0).sum()), int(picked.sum())
    log(f"{n_seen} of {P} Gaussians are the visible surface in some view; {n_picked} of them lie under the {views} masks of {W // 3} x {H // 3} pixels")
    assert 0 < n_picked <= n_seen, "no Gaussian under the masks"

    # 2. positions fitted to the median-depth maps of all views
    start = dict(truth)
    start["means3D"] = truth["means3D"] * 1.1               # what the optimiser has to undo: pushed outwards
    leaves, _flat, batch = batch_of(start)
    opt = FusedAdam([{"params": [leaves["means3D"]], "lr": 4e-3}])
    losses = []
    for step in range(steps + 1):
        depth, _index = step_of(leaves, batch)
        d = depth.detach().requires_grad_(True)
        loss = (d - target).abs().mean()
        (g,) = torch.autograd.grad(loss, d)
        batch.backward_median_views(g)
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
    ap.add_argument("--views", type=int, default=6)
    a = ap.parse_args()
    run(a.steps, a.gaussians, a.size[0], a.size[1], a.views)
