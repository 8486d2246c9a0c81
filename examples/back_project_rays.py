"""Ray casting for the editing region, on the device: what ``mesh_localization.py`` (:150-167) and ``back_project`` (``mask_mesh_0822.py`` :209-237) take from
``o3d.t.geometry.RaycastingScene``, without a rasterizer call:

  1. an icosphere (20 480 faces) and a pinhole camera: one ray per pixel of a disc-shaped mask, origin and direction as ``generate_back_projection_rays``
     hands them out, shape [1, M, 6];
  2. ``scene.hit_faces(rays)``: the reference's ``hit_tri_id_all_set`` as a bool [F] on the device, one launch, no host read-back; a second camera ORs into it;
  3. ``mesh_region.refine_region(faces, hit, V, 2, 5)``: the region the later stages edit;
  4. the same set once more the way the reference writes it -- ``cast_rays(rays)['primitive_ids']`` as numpy, a Python set of the ids below ``INVALID_ID`` --
     and the assertion that both routes give the same faces.

`python3 examples/back_project_rays.py [--subdivisions 5] [--size 256 256]` -- needs a HIP device."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def pinhole_rays(azimuth_deg, elevation_deg, distance, fov_deg, W, H, mask, device):
    """-> rays [1, M, 6] float32 through the centres of the pixels of ``mask`` [H,W] (origin, direction; the direction is not normalised)"""
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    back = torch.tensor([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)], dtype=torch.float64)
    right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), back)
    right = right / right.norm()
    up = torch.linalg.cross(back, right)
    yy, xx = torch.nonzero(mask.cpu(), as_tuple=True)
    half = math.tan(math.radians(fov_deg) / 2.0)
    x = ((xx.double() + 0.5) / W * 2.0 - 1.0) * half * (W / H)
    y = (1.0 - (yy.double() + 0.5) / H * 2.0) * half
    d = x[:, None] * right + y[:, None] * up - back                             # the camera looks along -back
    o = (distance * back).expand_as(d)
    return torch.cat([o, d], dim=1).float()[None].to(device)


def run(subdivisions=5, W=256, H=256, device="cuda", log=print):
    from youreditableavatar_amd import mesh_region, scenes
    from youreditableavatar_amd.mesh_rays import RaycastingScene
    dev = torch.device(device)
    v, f = scenes.icosphere(subdivisions)
    V, F = len(v), len(f)
    scene = RaycastingScene()
    assert scene.add_triangles(v, f) == 0                                       # numpy in, as the reference builds its scene; the tree is built once
    faces = torch.from_numpy(f).to(dev)

    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = (yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2 <= (0.12 * min(H, W)) ** 2
    rays = pinhole_rays(20.0, 10.0, 3.0, 40.0, W, H, disc, dev)
    other = pinhole_rays(35.0, 10.0, 3.0, 40.0, W, H, disc, dev)                # the next camera of the orbit

    hit = scene.hit_faces(rays)                                                 # the device route: no set, no host copy
    first = int(hit.sum())
    hit = scene.hit_faces(other, out=hit)                                       # hit |= the second camera's faces
    region = mesh_region.refine_region(faces, hit, V, dilate_iter=2, erode_iter=5)

    ids = set()                                                                 # the reference's route, line for line
    for r in (rays, other):
        ans = scene.cast_rays(r.cpu().numpy())
        hit_id = ans["primitive_ids"][0]
        ids |= set(hit_id[hit_id < RaycastingScene.INVALID_ID].tolist())
    on_device = set(torch.nonzero(hit)[:, 0].tolist())
    assert ids == on_device and 0 < first < len(ids) < F

    t = scene.cast_rays(rays)["t_hit"]
    seen = scene.test_occlusions(rays)
    assert torch.equal(seen, torch.isfinite(t)) and bool(seen.all())            # every pixel of the disc is on the sphere
    assert float((t - 2.0).abs().max()) < 0.1                                   # a unit sphere 3 away, seen near its centre, |d| about 1
    n_face, n_vert = int(region.face_mask.sum()), int(region.vertex_mask.sum())
    log(f"{F} faces, {rays.shape[1]} rays per camera at {W}x{H}: {first} faces hit by the first camera, {len(ids)} by both; refine_region(2, 5) keeps {n_face} faces on {n_vert} vertices")
    assert 0 < n_face and n_vert >= 3 and bool(region.vertex_mask[faces[region.face_mask].long()].all())
    return dict(hit=hit.cpu().numpy(), face_mask=region.face_mask.cpu().numpy(), vertex_mask=region.vertex_mask.cpu().numpy())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    a = ap.parse_args()
    run(a.subdivisions, a.size[0], a.size[1])
