#!/usr/bin/env python3
"""The head of the geometry stage's chain: a hash-grid SDF field fitted to a sphere, then one step of the whole chain with a gradient arriving in
the hash table.

``SdfField`` (``youreditableavatar_amd.hashgrid``) is ``forward_sdf`` of ``tetgs_spatial/models/geometry/implicit_sdf.py``: the box map, the hash-grid
encoding and the bias-free MLP in one kernel.  Part one fits it to the SDF of a sphere on the vertices of a small Kuhn grid (Adam on the table and
the two weight matrices).  Part two is the step the geometry stage takes: field -> ``marching_tets`` -> ``mesh_geom`` vertex normals ->
``mesh_raster_grad`` silhouette and normal map -> a loss, and ``backward()`` reaches ``encoding.params`` through every link.
Usage:  python examples/fit_hashgrid_sdf.py [--grid 16] [--resolution 96] [--steps 300]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONFIG = dict(otype="HashGrid", n_levels=8, n_features_per_level=2, log2_hashmap_size=14, base_resolution=4, per_level_scale=1.5)


def fit(grid=16, resolution=96, steps=300, lr=1e-2, device="cuda", verbose=True):
    import youreditableavatar_amd.mesh_raster_grad as dr
    from tests import mt_ref
    from youreditableavatar_amd import hashgrid, mesh_geom, scenes
    from youreditableavatar_amd.marching_tets import marching_tets
    dev = torch.device(device)
    torch.manual_seed(0)
    s = mt_ref.kuhn(int(grid))
    pos, tet = torch.from_numpy(s["pos"].copy()).to(dev), torch.from_numpy(s["tet"].copy()).to(dev)
    world = pos * 2.0 - 1.0                                                   # the stage's points live in [-1, 1]^3; the field maps them back
    encoding = hashgrid.HashGrid(3, CONFIG)
    mlp = torch.nn.Sequential(torch.nn.Linear(encoding.n_output_dims, 64, bias=False), torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 1, bias=False))
    field = hashgrid.SdfField(encoding, mlp, bbox=[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], bias=0.0).to(dev)
    assert field.fused
    target = 0.6 - world.norm(dim=1, keepdim=True)                            # positive inside, as marching_tets reads it
    opt = torch.optim.Adam(field.parameters(), lr=lr)
    first = last = None
    for step in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(field(world), target)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if verbose and (step % 50 == 0 or step == steps - 1):
            print(f"step {step:4d}  sdf mse {last:.6f}")

    # one step of the whole chain
    H = W = int(resolution)
    ctx = dr.RasterizeCudaContext(device=dev)
    proj = torch.from_numpy(np.asarray(scenes.orbit_camera(W, H, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0).projmatrix, np.float32)).to(dev)
    opt.zero_grad(set_to_none=True)
    sdf = field(world)[:, 0]
    mesh = marching_tets(pos, sdf, tet)
    verts = mesh["verts"] * 2.0 - 1.0
    topo = mesh_geom.mesh_topology(mesh["faces"], len(verts))
    normals = mesh_geom.vertex_normals(verts, mesh["faces"], topo)
    faces = mesh["faces"].int()
    clip = torch.nn.functional.pad(verts, pad=(0, 1), mode="constant", value=1.0) @ proj
    rast, _ = dr.rasterize(ctx, clip[None], faces, (H, W))
    mask = (rast[..., 3:] > 0).float()
    opacity = dr.antialias(mask, rast, clip, faces)
    shaded, _ = dr.interpolate(normals, rast, faces)
    chain_loss = opacity.mean() + 0.1 * (dr.antialias(shaded * mask, rast, clip, faces) ** 2).mean() + 0.05 * mesh_geom.normal_consistency(normals, topo)
    chain_loss.backward()
    g = encoding.params.grad
    res = dict(first_mse=first, last_mse=last, faces=len(faces), vertices=len(verts), covered_pixels=int(mask.sum()), chain_loss=float(chain_loss.detach()),
               params_grad_nonzero=int((g != 0).sum()), params_grad_finite=bool(torch.isfinite(g).all()), w1_grad_nonzero=int((mlp[0].weight.grad != 0).sum()))
    if verbose:
        print(f"sdf mse {first:.6f} -> {last:.6f} (factor {first / last:.1f}); the chain's step: {res['vertices']} vertices, {res['faces']} faces, {res['covered_pixels']} covered "
              f"pixels, loss {res['chain_loss']:.5f}, a gradient on {res['params_grad_nonzero']} of {g.numel()} table entries and {res['w1_grad_nonzero']} elements of W1")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=96)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    fit(a.grid, a.resolution, a.steps)
