#!/usr/bin/env python3
"""One camera of the painting stage's masks without leaving the device: ``prepare_mask_proj`` and ``back_project`` of
``tetgs_inpainter/mask_mesh_0822.py`` with ``mask_ops`` in the place of cv2 and ``mesh_region`` in the place of open3d and pymeshlab.

  1. an icosphere (20 480 faces) and an orbit camera from ``cameras.RasterCameras``  ->  ``dr.rasterize``;
  2. an edit disc in the image, as the antialiased mask of the stage: erode 2 -> dilate 20 -> blur 21 -> ``> 0`` gives ``mask_blur_binary``, and
     ``mask_proj`` is that under the rendered mesh (``mask_ops``; the reference goes through a PNG file and the host here);
  3. ``dr.hit_faces`` under ``mask_proj``: the faces ``back_project`` gets from ray casting;
  4. ``mesh_region.refine_region`` at (2, 5), the setting of the first eight cameras  ->  ``region.face_mask``, ``region.vertex_mask``;
     ``mask_dilate`` and ``verts_mask`` as the stage updates them; ``keep_large_components`` as the localisation cleans its region.

Prints the counts; asserts that the pieces agree with each other.
Usage:  python examples/paint_masks.py [--subdivisions 5] [--size 256 256]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def run(subdivisions=5, W=256, H=256, device="cuda", log=print):
    import youreditableavatar_amd.mesh_raster as dr
    from youreditableavatar_amd import mask_ops, mesh_region, scenes
    from youreditableavatar_amd.cameras import RasterCameras
    dev = torch.device(device)
    v, f = scenes.icosphere(subdivisions)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    V, F = len(v), len(f)
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
    covered = dr.face_ids(rast)[0] >= 0

    # the edit disc, three equal channels of 0 / 255 as cv2.imread returns the stage's mask
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = (yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2 <= (0.08 * min(H, W)) ** 2
    mask_aa = (disc[:, :, None].expand(H, W, 3) * 255).to(torch.uint8)
    mask_aa = mask_ops.erode(mask_aa, np.ones((2, 2), np.uint8))
    mask_blur = mask_ops.gaussian_blur(mask_ops.dilate(mask_aa, np.ones((20, 20), np.uint8)).float(), (21, 21), 0)
    mask_blur_binary = mask_blur[:, :, 0] > 0
    mask_proj = mask_blur_binary & covered

    hit = dr.hit_faces(rast, mask_proj, num_faces=F)
    region = mesh_region.refine_region(faces, hit, V, dilate_iter=2, erode_iter=5)
    mask_dilate = (~region.vertex_mask).float()[:, None]                        # 1: vertices to be updated, 0: kept
    verts_mask = torch.ones(V, dtype=torch.bool, device=dev)
    verts_mask &= ~region.vertex_mask
    kept = mesh_region.keep_large_components(region.face_mask, faces, V, int(0.25 * int(region.face_mask.sum())))

    n_disc, n_blur, n_proj, n_hit, n_face, n_vert = (int(x.sum()) for x in (disc, mask_blur_binary, mask_proj, hit, region.face_mask, region.vertex_mask))
    log(f"{F} faces at {W}x{H}: disc {n_disc} px -> mask_blur_binary {n_blur} px -> mask_proj {n_proj} px; {n_hit} faces hit, {n_face} after refine_region(2, 5) "
        f"on {n_vert} vertices; {int(kept.sum())} faces in components of at least a quarter")
    assert n_disc < n_blur and 0 < n_proj <= n_blur and 0 < n_hit < F
    assert bool(mask_blur_binary[disc].all())                                   # the blurred, dilated mask holds the disc
    assert 0 < n_face <= int(mesh_region.dilate_faces(hit, faces, V, 2).sum()) and n_vert >= 3
    assert bool(region.vertex_mask[faces[region.face_mask].long()].all()) and int(mask_dilate.sum()) == V - n_vert == int(verts_mask.sum())
    assert torch.equal(kept, region.face_mask)                                  # one blob: nothing is dropped
    return dict(mask_proj=mask_proj.cpu().numpy(), hit=hit.cpu().numpy(), face_mask=region.face_mask.cpu().numpy(), vertex_mask=region.vertex_mask.cpu().numpy())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    a = ap.parse_args()
    run(a.subdivisions, a.size[0], a.size[1])
