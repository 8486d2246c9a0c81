#!/usr/bin/env python3
"""The geometry stage in miniature: an SDF -> marching tetrahedra -> the mesh rasterizer -> an image loss, every step.

An SDF stored per vertex of a Kuhn grid (six tetrahedra per cube) goes through ``marching_tets`` -- the one line that
``MarchingTetrahedraHelper._forward`` (``tetgs_spatial/models/isosurface.py`` :112-184) becomes -- and the mesh through the three calls of
``youreditableavatar_amd.mesh_raster_grad`` from a few orbit cameras, as ``models/renderers/part_nvdiff_rasterizer.py`` :101-198 builds its
opacity and normal images.  The loss is a mask and normal loss against the images of a displaced, squeezed sphere; ``torch.optim.Adam`` moves
the SDF values.  The mesh changes its size from step to step (the numbers of vertices and faces are read back inside every call), and the
antialias topology is rebuilt inside every ``antialias`` call for the same reason.
Usage:  python examples/fit_sdf_silhouette.py [--grid 16] [--resolution 128] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from examples.fit_mesh_silhouette_normals import vertex_normals  # noqa: E402


def render(dr, ctx, verts, faces, proj, H, W):
    """world-space mesh (the grid's unit cube, recentred to [-1, 1]^3) -> opacity [1,H,W,1], comp_normal [1,H,W,3]"""
    world = verts * 2.0 - 1.0
    clip = torch.nn.functional.pad(world, pad=(0, 1), mode="constant", value=1.0) @ proj
    rast, _ = dr.rasterize(ctx, clip[None], faces, (H, W))
    mask = (rast[..., 3:] > 0).float()
    opacity = dr.antialias(mask, rast, clip, faces)
    normal, _ = dr.interpolate(vertex_normals(world, faces), rast, faces)
    normal = torch.lerp(torch.zeros_like(normal), (torch.nn.functional.normalize(normal, dim=-1) + 1.0) / 2.0, mask)
    return opacity, dr.antialias(normal, rast, clip, faces)


def fit(grid=16, resolution=128, steps=200, lr=2e-3, device="cuda", verbose=True):
    import youreditableavatar_amd.mesh_raster_grad as dr
    from tests import mt_ref
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.marching_tets import marching_tets
    dev = torch.device(device)
    H = W = int(resolution)
    s = mt_ref.kuhn(int(grid))
    pos, tet = torch.from_numpy(s["pos"].copy()).to(dev), torch.from_numpy(s["tet"].copy()).to(dev)
    ctx = dr.RasterizeCudaContext(device=dev)
    projs = [torch.from_numpy(np.asarray(scenes.orbit_camera(W, H, azimuth_deg=az, elevation_deg=el, radius=3.0, znear=1.0, zfar=10.0).projmatrix, np.float32)).to(dev)
             for az, el in ((25.0, 15.0), (145.0, -10.0), (265.0, 30.0))]

    def images(sdf):
        mesh = marching_tets(pos, sdf, tet)
        faces = mesh["faces"].int()
        return [render(dr, ctx, mesh["verts"], faces, p, H, W) for p in projs], mesh

    centre, squeeze = torch.tensor([0.55, 0.47, 0.5], device=dev), torch.tensor([1.2, 0.85, 1.0], device=dev)
    with torch.no_grad():
        want, target_mesh = images(0.33 - ((pos - centre) / squeeze).norm(dim=1))
    sdf = (0.3 - (pos - 0.5).norm(dim=1)).requires_grad_(True)
    opt = torch.optim.Adam([sdf], lr=lr)
    first = last = None
    sizes = set()
    for step in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        got, mesh = images(sdf)
        sizes.add((len(mesh["verts"]), len(mesh["faces"])))
        loss = sum(torch.nn.functional.mse_loss(o, wo) + torch.nn.functional.mse_loss(n, wn) for (o, n), (wo, wn) in zip(got, want))
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if verbose and (step % 10 == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {last:.6f}  mesh {len(mesh['verts'])} vertices, {len(mesh['faces'])} faces")
    res = dict(first_loss=first, last_loss=last, mesh_sizes_seen=len(sizes), target_faces=len(target_mesh["faces"]), last_faces=len(mesh["faces"]))
    if verbose:
        print(f"{len(tet)} tetrahedra, {len(projs)} cameras at {W}x{H}: loss {first:.6f} -> {last:.6f} (factor {first / last:.2f}); {len(sizes)} different mesh sizes in "
              f"{steps} steps, the target has {res['target_faces']} faces, the last mesh {res['last_faces']}")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    fit(a.grid, a.resolution, a.steps)
