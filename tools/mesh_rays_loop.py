"""What ray casting for the editing region costs (youreditableavatar_amd.mesh_rays, csrc/tgs_mesh_rays.hip): ``cast_rays`` and ``hit_faces`` for the
1024 x 1024 rays of one pinhole camera, on the body mesh of tests/golden/ref_mesh_sdf_fixture.npz (20 908 faces) through the tree (mode 0) and over every face
(mode 1), and on the icosphere of tools/mesh_raster_loop.py scaled to 0.9 (1 310 720 faces) through the tree; ``test_occlusions`` beside them; and the existing
route to the same face set for the same camera, ``dr.rasterize`` plus ``dr.hit_faces`` under a full mask.  There is no earlier implementation of the ray
route on this hardware and open3d is not installed: nothing stands beside these figures but the rasterizer route.

`python3 tools/mesh_rays_loop.py [calls per block] [rounds] [subdivisions of the icosphere] [output file]` -- the protocol of tools/mesh_sdf_loop.py: per
case a warm-up of 10 calls (2 for mode 1), then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time
per call, with the spread of the blocks beside it.  A record, not a bar.  The tool asserts that mode 0 and mode 1 give the same bits
on the body mesh before it times anything.  The two routes sample a pixel differently (a ray through its centre; the rasterizer's coverage rule), so
their face sets are reported with their overlap, not asserted equal."""
import json, math, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import youreditableavatar_amd.mesh_raster as dr
from tests import mesh_sdf_ref
from youreditableavatar_amd import build, scenes
from youreditableavatar_amd.cameras import RasterCameras
from youreditableavatar_amd.mesh_rays import RaycastingScene
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
subdiv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
out_path = sys.argv[4] if len(sys.argv) > 4 else None
H = W = 1024
dev = torch.device("cuda", 0)


def timed(fn, warm=10, calls=calls):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / calls * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


# one camera: 20 degrees round, 10 up, 3 away, 40 degrees of view
az, el, fov = math.radians(20.0), math.radians(10.0), math.radians(40.0)
back = np.array([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
right = np.cross([0.0, 1.0, 0.0], back); right /= np.linalg.norm(right)
up = np.cross(back, right)
c2w = np.concatenate([np.stack([right, up, back], 1), (3.0 * back)[:, None]], 1)[None].astype(np.float32)
cams = RasterCameras.from_camera_to_worlds(c2w, znear=1.0, zfar=10.0, fov_x=fov, fov_y=fov, image_height=H, image_width=W, device=dev)
half = math.tan(fov / 2.0)
ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
d = (((xs + 0.5) / W * 2.0 - 1.0) * half)[..., None] * torch.from_numpy(right) + ((1.0 - (ys + 0.5) / H * 2.0) * half)[..., None] * torch.from_numpy(up) - torch.from_numpy(back)
rays = torch.cat([torch.from_numpy(3.0 * back).expand_as(d), d], dim=-1).float().to(dev)          # [H, W, 6]
glctx = dr.RasterizeCudaContext(device=dev)
full = torch.ones((H, W), dtype=torch.bool, device=dev)
res = {"calls_per_block": calls, "rounds": rounds, "rays": H * W, "library": build.source_hash(), "cases": {}}


def case_of(name, v, f, with_every_face):
    t0 = time.perf_counter()
    scene = RaycastingScene(v, f)
    case = {"vertices": len(v), "faces": len(f), "host_build_with_upload_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    if with_every_face:                                                         # before anything is timed
        a, b = scene.cast_rays(rays, mode=0), scene.cast_rays(rays, mode=1)
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and torch.equal(scene.hit_faces(rays, mode=0), scene.hit_faces(rays, mode=1))
        assert torch.equal(scene.test_occlusions(rays, mode=0), scene.test_occlusions(rays, mode=1))
    out = scene.cast_rays(rays)
    hit = scene.hit_faces(rays)
    want = torch.zeros(len(f), dtype=torch.bool, device=dev)
    want[out["primitive_ids"][out["primitive_ids"] >= 0].long()] = True
    assert torch.equal(hit, want)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    clip = torch.matmul(torch.nn.functional.pad(verts, pad=(0, 1), mode="constant", value=1.0), cams.projmatrix[0]).float().unsqueeze(0)
    raster_route = lambda: dr.hit_faces(dr.rasterize(glctx, clip, faces, (H, W))[0], full, num_faces=len(f))
    by_raster = raster_route()
    case.update(hit_share_of_rays=round(float((out["primitive_ids"] >= 0).float().mean()), 4), faces_hit=int(hit.sum()), faces_hit_by_the_raster_route=int(by_raster.sum()),
                faces_hit_by_both=int((hit & by_raster).sum()))
    case["cast_rays_tree"] = timed(lambda: scene.cast_rays(rays))
    case["hit_faces_tree"] = timed(lambda: scene.hit_faces(rays))
    case["test_occlusions_tree"] = timed(lambda: scene.test_occlusions(rays))
    if with_every_face:
        case["cast_rays_every_face"] = timed(lambda: scene.cast_rays(rays, mode=1), warm=2, calls=max(1, calls // 5))
    case["rasterize_plus_hit_faces"] = timed(raster_route)
    case["rasterize_alone"] = timed(lambda: dr.rasterize(glctx, clip, faces, (H, W)))
    res["cases"][name] = case
    print(json.dumps({name: case}), flush=True)


body_v, body_f = mesh_sdf_ref.load_fixture()[:2]
case_of("body", body_v, body_f, True)
ico_v, ico_f = scenes.icosphere(subdiv)
case_of(f"icosphere_{subdiv}", (ico_v * np.float32(0.9)).astype(np.float32), ico_f, False)
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
