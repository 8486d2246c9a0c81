#!/usr/bin/env python3
"""The three calls of the painting stage on its mesh rasterizer: ``import youreditableavatar_amd.mesh_raster_aa as dr`` in the place of the
third-party module of ``tetgs_inpainter/mask_mesh_0822.py``, with no call-site edits.

  1. the icosphere and the orbit camera of ``examples/mesh_masks.py``  ->  clip-space vertices, as ``mask_mesh`` :93 builds them;
  2. ``dr.rasterize``  ->  rast;  ``dr.interpolate`` of a vertex mask (the vertices of the upper half), as ``mask_mesh`` :97 does;
  3. ``dr.antialias(mask.float(), rast, vertices_clip, faces)`` as at :98, with the topology built once
     (``dr.antialias_construct_topology_hash``), thresholded with ``> 0`` like every mask of that stage.

Prints how many mask pixels the blend adds: what INTEGRATION.md 4j's edits lose.  The finer the mesh, the fewer: a silhouette is found through
the triangle a pixel shows, and limb triangles thinner than a pixel show in few pixels (try --subdivisions 2).
Usage:  python examples/mesh_masks_antialias.py [--subdivisions 4] [--size 256 256]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(subdivisions=4, W=256, H=256, device="cuda", log=print):
    import youreditableavatar_amd.mesh_raster_aa as dr
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.cameras import RasterCameras
    dev = torch.device(device)
    v, f = scenes.icosphere(subdivisions)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    az, el = math.radians(20.0), math.radians(10.0)
    back = np.array([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
    right = np.cross([0.0, 1.0, 0.0], back); right /= np.linalg.norm(right)
    up = np.cross(back, right)
    c2w = np.concatenate([np.stack([right, up, back], 1), (3.0 * back)[:, None]], 1)[None].astype(np.float32)
    fov = math.radians(40.0)
    cams = RasterCameras.from_camera_to_worlds(c2w, znear=1.0, zfar=10.0, fov_x=fov, fov_y=fov, image_height=H, image_width=W, device=dev)

    glctx = dr.RasterizeCudaContext(device=dev)
    vertices_clip = torch.matmul(torch.nn.functional.pad(verts, pad=(0, 1), mode="constant", value=1.0), cams.projmatrix[0]).float().unsqueeze(0)
    rast, _ = dr.rasterize(glctx, vertices_clip, faces, (H, W))
    verts_mask = (verts[:, 1:2] > 0).float().contiguous()                       # [V,1]: the upper half of the sphere
    mask, _ = dr.interpolate(verts_mask.unsqueeze(0), rast, faces)
    mask = (mask > 0)

    topology = dr.antialias_construct_topology_hash(faces)                      # once per mesh
    mask_aa = dr.antialias(mask.float(), rast, vertices_clip, faces, topology_hash=topology)
    after = mask_aa > 0

    n_before, n_after = int(mask.sum()), int(after.sum())
    log(f"{len(f)} faces at {W}x{H}: {n_before} pixels under the vertex mask")
    log(f"antialias blends {int((mask_aa != mask.float()).sum())} pixels and adds {n_after - n_before} mask pixels")
    assert bool((after | ~mask).all()) and n_after > n_before                    # the mask only grows
    assert bool((mask_aa >= 0).all())                                           # blends of 0 and 1
    return dict(pos=vertices_clip[0].cpu().numpy(), tri=f, rast=rast[0].cpu().numpy(), mask=mask[0].float().cpu().numpy(),
                mask_aa=mask_aa[0].cpu().numpy(), added=n_after - n_before)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    a = ap.parse_args()
    run(a.subdivisions, a.size[0], a.size[1])
