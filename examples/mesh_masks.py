#!/usr/bin/env python3
"""The mesh masks of the painting stage without a CUDA rasterizer: ``import youreditableavatar_amd.mesh_raster as dr`` in the place of the
third-party module of ``tetgs_inpainter/mask_mesh_0822.py``.

  1. an icosphere (5 120 faces) and an orbit camera from ``cameras.RasterCameras``  ->  clip-space vertices, as ``mask_mesh`` :93 builds them;
  2. ``dr.rasterize``  ->  rast [1,H,W,4] = (u, v, z/w, face + 1);
  3. ``dr.interpolate`` of a vertex mask (the vertices of the upper half) and of the vertex normals, as ``mask_mesh`` :97 / :107 do; the mask is
     thresholded with ``> 0`` like every mask of that stage (no ``antialias``: INTEGRATION.md 4j);
  4. ``dr.hit_faces`` under a 2-D mask (a rectangle in the middle of the image): the faces ``back_project`` gets from ray casting.

Prints the counts; asserts that the pieces agree with each other.
Usage:  python examples/mesh_masks.py [--subdivisions 4] [--size 256 256]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(subdivisions=4, W=256, H=256, device="cuda", log=print):
    import youreditableavatar_amd.mesh_raster as dr
    from youreditableavatar_amd import scenes
    from youreditableavatar_amd.cameras import RasterCameras
    dev = torch.device(device)
    v, f = scenes.icosphere(subdivisions)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    # one orbit camera, 3 units from the centre, 20 degrees round and 10 up (OpenGL camera-to-world: x right, y up, z back)
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
    mask = mask[0] > 0
    normals, _ = dr.interpolate(verts, rast, faces)                             # a unit sphere's vertex normals are its vertices; [V,3] broadcasts
    ids = dr.face_ids(rast)[0]
    covered = ids >= 0

    rect = torch.zeros((H, W), dtype=torch.bool, device=dev)
    rect[H // 3:2 * H // 3, W // 3:2 * W // 3] = True
    hit = dr.hit_faces(rast, rect, num_faces=len(f))

    n_cov, n_mask, n_hit = int(covered.sum()), int(mask.sum()), int(hit.sum())
    log(f"{len(f)} faces at {W}x{H}: {n_cov} pixels covered, {n_mask} under the vertex mask, {n_hit} faces hit under the rectangle")
    assert 0 < n_mask < n_cov < H * W and 0 < n_hit < len(f)
    assert not bool(mask[..., 0][~covered].any())                                # a mask exists on the mesh only
    length = normals[0].norm(dim=-1)
    assert bool(((length[covered] - 1).abs() < 0.01).all()) and bool((length[~covered] == 0).all())
    assert bool((ids[rect][ids[rect] >= 0].unique() == hit.nonzero()[:, 0]).all())
    return dict(pos=vertices_clip[0].cpu().numpy(), tri=f, rast=rast[0].cpu().numpy(), rect=rect.cpu().numpy(), hit=hit.cpu().numpy(),
                mask=mask.cpu().numpy(), normals=normals[0].cpu().numpy())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    a = ap.parse_args()
    run(a.subdivisions, a.size[0], a.size[1])
