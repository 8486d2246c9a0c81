#!/usr/bin/env python3
"""Stage 0 of the geometry pipeline in miniature: a hash-grid SDF field fitted to the signed distance of a mesh, then the field's surface.

``ImplicitSDF.initialize_shape`` (``tetgs_spatial/models/geometry/implicit_sdf.py`` :172-339) loads the body mesh, centres and scales it, and runs
15 000 iterations of: draw uniform points in [-1, 1]^3, take their signed distance to the mesh, evaluate the field, MSE, Adam.  Here the mesh is an
icosphere with a dent (no file is read), ``mesh_sdf.SDF`` is the target -- a device tensor in, a device tensor out, nothing goes through the host --
``hashgrid.SdfField`` is the field, and after a few hundred iterations the field on the vertices of a Kuhn grid goes to ``marching_tets``.
Usage:  python examples/init_sdf_from_mesh.py [--steps 300] [--points 40000] [--grid 32]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONFIG = dict(otype="HashGrid", n_levels=8, n_features_per_level=2, log2_hashmap_size=15, base_resolution=4, per_level_scale=1.5)


def fit(steps=300, points=40000, grid=32, lr=1e-2, device="cuda", verbose=True):
    from tests import mesh_sdf_ref, mt_ref
    from youreditableavatar_amd import hashgrid
    from youreditableavatar_amd.marching_tets import marching_tets
    from youreditableavatar_amd.mesh_sdf import SDF
    dev = torch.device(device)
    torch.manual_seed(0)
    vertices, faces = mesh_sdf_ref.icosphere(3, dent=0.35)                       # 1 280 faces
    vertices = vertices.astype(np.float64) + np.array([0.2, -0.1, 0.05])         # a mesh as a file gives it: somewhere, at some size
    # lines 202-229 inline: the centroid to the origin, the reference's shift, the largest |coordinate| to shape_init_params = 0.9 (up +z, front +x: no turn)
    vertices = vertices - vertices.mean(0)
    vertices[:, 1] = vertices[:, 1] + 0.3
    vertices = vertices / np.abs(vertices).max() * 0.9
    sdf = SDF(vertices, faces)                                                   # built once; vertices, faces and the tree stay on the device
    get_gt_sdf = lambda points_rand: -sdf(points_rand)[..., None]                # the reference's sign: negative inside
    encoding = hashgrid.HashGrid(3, CONFIG)
    mlp = torch.nn.Sequential(torch.nn.Linear(encoding.n_output_dims, 64, bias=False), torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 1, bias=False))
    field = hashgrid.SdfField(encoding, mlp, bbox=[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], bias=0.0).to(dev)
    optim = torch.optim.Adam(field.parameters(), lr=lr)
    first = last = None
    for step in range(int(steps)):
        points_rand = torch.rand((int(points), 3), dtype=torch.float32, device=dev) * 2.0 - 1.0
        loss = torch.nn.functional.mse_loss(field(points_rand), get_gt_sdf(points_rand))
        optim.zero_grad(set_to_none=True)
        loss.backward()
        optim.step()
        last = float(loss.detach())
        first = last if first is None else first
        if verbose and (step % 50 == 0 or step == steps - 1):
            print(f"step {step:4d}  sdf mse {last:.6f}")

    s = mt_ref.kuhn(int(grid))
    pos, tet = torch.from_numpy(s["pos"].copy()).to(dev), torch.from_numpy(s["tet"].copy()).to(dev)
    world = pos * 2.0 - 1.0
    with torch.no_grad():
        mesh = marching_tets(pos, -field(world)[:, 0], tet)                       # marching_tets reads positive inside
        surface = mesh["verts"] * 2.0 - 1.0
        off = sdf(surface).abs() if len(surface) else torch.zeros(0, device=dev)  # how far the field's surface lies from the mesh it was fitted to
    res = dict(first_mse=first, last_mse=last, vertices=len(surface), faces=len(mesh["faces"]), mean_distance_to_the_mesh=float(off.mean()) if len(off) else float("nan"),
               max_distance_to_the_mesh=float(off.max()) if len(off) else float("nan"), inside_share=float(sdf.contains(world).float().mean()))
    if verbose:
        print(f"sdf mse {first:.6f} -> {last:.6f} (factor {first / last:.1f}); the field's surface on a {grid}^3 grid: {res['vertices']} vertices, {res['faces']} faces, "
              f"{res['mean_distance_to_the_mesh']:.4f} from the mesh on average, {res['max_distance_to_the_mesh']:.4f} at most (a grid cell is {2.0 / grid:.4f})")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--grid", type=int, default=32)
    a = ap.parse_args()
    r = fit(a.steps, a.points, a.grid)
    assert r["last_mse"] < 0.1 * r["first_mse"] and r["faces"] > 0, r
