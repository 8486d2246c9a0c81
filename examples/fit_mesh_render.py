#!/usr/bin/env python3
"""An optimisation step of the geometry stage on its fused renderer body: ``youreditableavatar_amd.mesh_shade.render`` in the place of
``models/renderers/part_nvdiff_rasterizer.py`` :100-152.

The vertices of a 320-face icosphere are moved towards the mask and the camera-space normal image of a displaced one.  Every step is

    out  = render(ctx, verts, faces, mvp, (H, W), normal_type="camera", c2w=c2w, topology_hash=topology)
    loss = mse(out["opacity"], want_opacity) + mse(out["comp_normal"], want_normal)

with no read-back inside ``render``: the camera matrix is inverted in the kernel, the indices are not validated per call, and the two topologies
of the mesh are built once, outside the loop.
The mask loss reaches the vertices through ``antialias`` (the silhouette gradient); the normal loss through the vertex normals, through
``rasterize``'s u, v, and through ``antialias``.
Usage:  python examples/fit_mesh_render.py [--resolution 256] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def fit(resolution=256, steps=200, lr=4e-3, device="cuda", verbose=True):
    import youreditableavatar_amd.mesh_raster_grad as dr
    from youreditableavatar_amd import mesh_geom, mesh_shade, scenes
    dev = torch.device(device)
    H = W = int(resolution)
    v, f = scenes.icosphere(2)                                                   # 320 faces
    cam = scenes.orbit_camera(W, H, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    mvp = torch.from_numpy(np.ascontiguousarray(np.asarray(cam.projmatrix, np.float32).T)).to(dev)[None]      # pos_clip = [verts, 1] @ mvp^T
    c2w = torch.from_numpy(np.linalg.inv(np.asarray(cam.viewmatrix, np.float64).T).astype(np.float32)).to(dev)[None]
    faces = torch.from_numpy(f).to(dev)
    ctx = dr.RasterizeCudaContext(device=dev)
    topology = dr.antialias_construct_topology_hash(faces)                       # once per mesh, both of them
    incidence = mesh_geom.mesh_topology(faces, len(v), edges=False)

    def render(verts):
        return mesh_shade.render(ctx, verts, faces, mvp, (H, W), normal_type="camera", c2w=c2w, depth=False, topology_hash=topology,
                                 normals_topology=incidence)
    target_verts = torch.from_numpy(v).to(dev) * torch.tensor([1.15, 0.85, 1.0], device=dev) + torch.tensor([0.08, -0.05, 0.0], device=dev)
    with torch.no_grad():
        want = render(target_verts)
    verts = torch.from_numpy(v).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([verts], lr=lr)
    first = last = None
    for step in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        out = render(verts)
        loss = torch.nn.functional.mse_loss(out["opacity"], want["opacity"]) + torch.nn.functional.mse_loss(out["comp_normal"], want["comp_normal"])
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if verbose and (step % 20 == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {last:.6f}")
    if verbose:
        print(f"{len(f)} faces at {W}x{H}: loss {first:.6f} -> {last:.6f} (factor {first / last:.2f})")
    return dict(first_loss=first, last_loss=last)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    fit(a.resolution, a.steps)
