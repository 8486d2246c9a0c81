#!/usr/bin/env python3
"""The geometry stage in miniature, without one framework scatter: an SDF -> marching tetrahedra -> vertex normals -> the mesh rasterizer -> an
image loss plus the normal-consistency loss, every step.

The setup is ``examples/fit_sdf_silhouette.py``'s: an SDF per vertex of a Kuhn grid, ``marching_tets``, a few orbit cameras, a mask and normal
loss against the images of a displaced, squeezed sphere.  Here the normal map comes from ``youreditableavatar_amd.mesh_geom.vertex_normals`` (the
body of ``compute_normal``, ``tetgs_spatial/models/renderers/nvdiff_rasterize_utils.py`` :12-35) through ``interpolate``, and the loss adds
``mesh_normal_consistency`` (``out["update_mesh"].normal_consistency()``, ``systems/humanedit.py`` :205-216) on the same topology, which is built once
per step because the mesh is new every step.
Usage:  python examples/fit_sdf_normals.py [--grid 16] [--resolution 128] [--steps 200] [--lambda-nc 0.05]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def render(dr, ctx, world, normals, faces, proj, H, W):
    """world-space mesh in [-1, 1]^3 and its vertex normals -> opacity [1,H,W,1], comp_normal [1,H,W,3]"""
    clip = torch.nn.functional.pad(world, pad=(0, 1), mode="constant", value=1.0) @ proj
    rast, _ = dr.rasterize(ctx, clip[None], faces, (H, W))
    mask = (rast[..., 3:] > 0).float()
    opacity = dr.antialias(mask, rast, clip, faces)
    normal, _ = dr.interpolate(normals, rast, faces)
    normal = torch.lerp(torch.zeros_like(normal), (torch.nn.functional.normalize(normal, dim=-1) + 1.0) / 2.0, mask)
    return opacity, dr.antialias(normal, rast, clip, faces)


def fit(grid=16, resolution=128, steps=200, lr=2e-3, lambda_nc=0.05, device="cuda", verbose=True):
    import youreditableavatar_amd.mesh_raster_grad as dr
    from tests import mt_ref
    from youreditableavatar_amd import mesh_geom, scenes
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
        world = mesh["verts"] * 2.0 - 1.0                                     # the grid's unit cube, recentred
        topo = mesh_geom.mesh_topology(mesh["faces"], len(world))             # once per mesh: the normals and the loss share it
        normals = mesh_geom.vertex_normals(world, mesh["faces"], topo)
        faces = mesh["faces"].int()
        return [render(dr, ctx, world, normals, faces, p, H, W) for p in projs], mesh_geom.normal_consistency(normals, topo), mesh

    centre, squeeze = torch.tensor([0.55, 0.47, 0.5], device=dev), torch.tensor([1.2, 0.85, 1.0], device=dev)
    with torch.no_grad():
        want, _, target_mesh = images(0.33 - ((pos - centre) / squeeze).norm(dim=1))
    sdf = (0.3 - (pos - 0.5).norm(dim=1)).requires_grad_(True)
    opt = torch.optim.Adam([sdf], lr=lr)
    first = last = first_nc = last_nc = None
    sizes = set()
    for step in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        got, nc, mesh = images(sdf)
        sizes.add((len(mesh["verts"]), len(mesh["faces"])))
        loss = sum(torch.nn.functional.mse_loss(o, wo) + torch.nn.functional.mse_loss(n, wn) for (o, n), (wo, wn) in zip(got, want)) + lambda_nc * nc
        loss.backward()
        opt.step()
        last, last_nc = float(loss.detach()), float(nc.detach())
        first, first_nc = (last, last_nc) if first is None else (first, first_nc)
        if verbose and (step % 10 == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {last:.6f}  normal consistency {last_nc:.5f}  mesh {len(mesh['verts'])} vertices, {len(mesh['faces'])} faces")
    res = dict(first_loss=first, last_loss=last, first_consistency=first_nc, last_consistency=last_nc, mesh_sizes_seen=len(sizes),
               target_faces=len(target_mesh["faces"]), last_faces=len(mesh["faces"]))
    if verbose:
        print(f"{len(tet)} tetrahedra, {len(projs)} cameras at {W}x{H}: loss {first:.6f} -> {last:.6f} (factor {first / last:.2f}), normal consistency {first_nc:.5f} -> "
              f"{last_nc:.5f}; {len(sizes)} different mesh sizes in {steps} steps, the target has {res['target_faces']} faces, the last mesh {res['last_faces']}")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lambda-nc", type=float, default=0.05)
    a = ap.parse_args()
    fit(a.grid, a.resolution, a.steps, lambda_nc=a.lambda_nc)
