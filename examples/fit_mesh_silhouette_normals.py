#!/usr/bin/env python3
"""An optimisation step of the geometry stage on its mesh rasterizer: ``import youreditableavatar_amd.mesh_raster_grad as dr`` in the place of the
third-party module of ``tetgs_spatial/utils/rasterize.py``.

The vertices of a 320-face icosphere are moved towards the mask and the normal image of a displaced one, through the images
``models/renderers/part_nvdiff_rasterizer.py`` :101-198 builds:

    rast                   = dr.rasterize(ctx, v_pos_clip, faces, (H, W))
    opacity                = dr.antialias(mask, rast, v_pos_clip, faces)                      mask = rast[..., 3:] > 0
    comp_normal            = dr.antialias(lerp(0, (normalize(dr.interpolate(vn, rast, faces)) + 1) / 2, mask), rast, v_pos_clip, faces)

The mask loss reaches the vertices through ``antialias`` alone (the silhouette gradient); the normal loss through ``interpolate``'s attributes
(the vertex normals are a function of the vertices) and through ``rasterize``'s u, v.
Usage:  python examples/fit_mesh_silhouette_normals.py [--resolution 256] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def vertex_normals(verts, faces):
    """area-weighted vertex normals, differentiable in ``verts``"""
    f = faces.long()
    v0, v1, v2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    fn = torch.cross(v1 - v0, v2 - v0, dim=-1)
    vn = torch.zeros_like(verts).index_add(0, f.reshape(-1), fn.repeat_interleave(3, dim=0))
    return torch.nn.functional.normalize(vn, dim=-1)


def render(dr, ctx, verts, faces, proj, topology, H, W):
    """-> opacity [1,H,W,1], comp_normal [1,H,W,3], v_pos_clip [V,4]"""
    clip = torch.nn.functional.pad(verts, pad=(0, 1), mode="constant", value=1.0) @ proj
    rast, _ = dr.rasterize(ctx, clip[None], faces, (H, W))
    mask = (rast[..., 3:] > 0).float()
    opacity = dr.antialias(mask, rast, clip, faces, topology_hash=topology)
    normal, _ = dr.interpolate(vertex_normals(verts, faces), rast, faces)
    normal = torch.lerp(torch.zeros_like(normal), (torch.nn.functional.normalize(normal, dim=-1) + 1.0) / 2.0, mask)
    return opacity, dr.antialias(normal, rast, clip, faces, topology_hash=topology), clip


def fit(resolution=256, steps=200, lr=4e-3, device="cuda", verbose=True):
    import youreditableavatar_amd.mesh_raster_grad as dr
    from youreditableavatar_amd import scenes
    dev = torch.device(device)
    H = W = int(resolution)
    v, f = scenes.icosphere(2)                                                   # 320 faces
    cam = scenes.orbit_camera(W, H, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    proj = torch.from_numpy(np.asarray(cam.projmatrix, np.float32)).to(dev)
    faces = torch.from_numpy(f).to(dev)
    ctx = dr.RasterizeCudaContext(device=dev)
    topology = dr.antialias_construct_topology_hash(faces)                       # once per mesh
    target_verts = torch.from_numpy(v).to(dev) * torch.tensor([1.15, 0.85, 1.0], device=dev) + torch.tensor([0.08, -0.05, 0.0], device=dev)
    with torch.no_grad():
        want_opacity, want_normal, _ = render(dr, ctx, target_verts, faces, proj, topology, H, W)
    verts = torch.from_numpy(v).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([verts], lr=lr)

    # the silhouette gradient on its own: under the mask loss, antialias is the only path to the vertices
    opacity, _, clip = render(dr, ctx, verts, faces, proj, topology, H, W)
    (d_clip,) = torch.autograd.grad(torch.nn.functional.mse_loss(opacity, want_opacity), clip)
    moved = d_clip.abs().sum(dim=1) > 0
    X = clip[:, :2].detach() / clip[:, 3:].detach()
    t = faces.long()
    front = ((X[t[:, 1], 0] - X[t[:, 0], 0]) * (X[t[:, 2], 1] - X[t[:, 0], 1]) - (X[t[:, 2], 0] - X[t[:, 0], 0]) * (X[t[:, 1], 1] - X[t[:, 0], 1])) > 0
    on_front, on_back = torch.zeros(len(v), dtype=torch.bool, device=dev), torch.zeros(len(v), dtype=torch.bool, device=dev)
    on_front[t[front].reshape(-1)] = True
    on_back[t[~front].reshape(-1)] = True
    limb = on_front & on_back                                                    # vertices of an edge between a front and a back face

    first = last = None
    for step in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        opacity, normal, _ = render(dr, ctx, verts, faces, proj, topology, H, W)
        loss = torch.nn.functional.mse_loss(opacity, want_opacity) + torch.nn.functional.mse_loss(normal, want_normal)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if verbose and (step % 20 == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {last:.6f}")
    res = dict(first_loss=first, last_loss=last, silhouette_vertices=int(limb.sum()), silhouette_grad_nonzero=int((moved & limb).sum()),
               grad_rows_nonzero=int(moved.sum()))
    if verbose:
        print(f"{len(f)} faces at {W}x{H}: loss {first:.6f} -> {last:.6f} (factor {first / last:.2f}); the mask loss alone moves {res['grad_rows_nonzero']} vertices, "
              f"{res['silhouette_grad_nonzero']} of the {res['silhouette_vertices']} on the limb")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    fit(a.resolution, a.steps)
