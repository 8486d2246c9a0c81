#!/usr/bin/env python3
"""Fitting per-Gaussian feature channels and opacities to target maps with the rasterizer's feature output
(``GaussianRasterizer(...)(..., features=F)``: feature_map[C,H,W] = sum_i T_i alpha_i F[i, :], differentiable through F and through alpha):

  a cloud with a 4-channel feature per Gaussian -- a signed unit "normal" (3) and an edit mask (1) -- whose features were scrambled and
  whose opacities were faded  ->  the feature map of one view through the drop-in API  ->  loss = l1_loss(feature_map, target) against the
  original cloud's map  ->  autograd  ->  Adam on the features and the opacities.

The image takes no part in the loss: one backward call carries the map's upstream gradient alone.  Asserts that the loss falls; prints it
at steps 0 and N.
Usage:  python examples/fit_features.py [--steps 40] [--gaussians 5000] [--size 160 120]
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
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    normals = rng.standard_normal((P, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)                # signed: half of the components are negative
    mask = (np.asarray(cloud["means3D"])[:, :1] > np.median(np.asarray(cloud["means3D"])[:, 0])).astype(np.float64)      # "edit" half of the cloud
    truth_feat = t(np.concatenate([normals, mask], 1))
    c = scenes.orbit_camera(W, H, azimuth_deg=20.0, bg=(0.0, 0.0, 0.0))
    rasterizer = GaussianRasterizer(GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(c.bg), scale_modifier=1.0, viewmatrix=t(c.viewmatrix),
        projmatrix=t(c.projmatrix), sh_degree=int(cloud["sh_degree"]), campos=t(c.campos), prefiltered=False, debug=False))

    def render(opacities, features):
        _color, _radii, fmap = rasterizer(means3D=truth["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True), opacities=opacities,
                                          shs=truth["shs"], scales=truth["scales"], rotations=truth["rotations"], features=features)
        return fmap

    with torch.no_grad():
        target = render(truth["opacities"], truth_feat).clone()
    feat = (0.3 * truth_feat + 0.5 * t(rng.standard_normal((P, 4)))).requires_grad_(True)       # what the optimiser has to undo: scrambled ...
    opac = (truth["opacities"] * 0.6).clamp(0.02, 0.99).requires_grad_(True)                    # ... and faded
    opt = torch.optim.Adam([{"params": [feat], "lr": 5e-2}, {"params": [opac], "lr": 2e-2}])
    losses = []
    for step in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        loss = l1_loss(render(opac, feat), target)
        loss.backward()
        losses.append(loss.detach())                        # (a device tensor: no host sync inside the step)
        if step < steps:
            opt.step()
            with torch.no_grad():
                opac.clamp_(0.01, 0.99)
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
