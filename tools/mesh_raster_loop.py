"""What the mesh rasterizer costs: `rasterize` and `interpolate` (youreditableavatar_amd.mesh_raster, csrc/tgs_mesh.hip) for a subdivided sphere of
1 310 720 faces (8 subdivisions of the icosahedron: the size of an avatar mesh) through an orbit camera, at 1024 x 1024 and 2048 x 2048, and once more
for a screen-filling pair of triangles at each size (the large-triangle path: it must cost about what a screen of small ones costs).

`python3 tools/mesh_raster_loop.py [calls per block] [rounds] [subdivisions]` -- per case a warm-up of 10 calls, then `rounds` blocks of `calls`
calls each between two synchronisations; the figure is the median block's time per call, with the spread of the blocks beside it.  There is no
earlier implementation to compare with on this hardware: the output is a record, not a bar.  Under
`rocprofv3 --kernel-trace --stats -- python3 tools/mesh_raster_loop.py ...` the per-kernel times of k_mesh_clear / _small / _large / _resolve /
_interpolate."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
import youreditableavatar_amd.mesh_raster as dr
from youreditableavatar_amd import build, scenes
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
subdiv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
dev = torch.device("cuda", 0)
verts_np, faces_np = scenes.icosphere(subdiv)
verts, faces = torch.from_numpy(verts_np).to(dev), torch.from_numpy(faces_np).to(dev)
pair_faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
pair_pos = torch.tensor([[[-1.1, -1.1, 0.1, 1.0], [2.2, -2.2, 0.6, 2.0], [1.65, 1.65, 0.75, 1.5], [-0.88, 0.88, 0.16, 0.8]]], device=dev)
glctx = dr.RasterizeCudaContext(device=dev)


def timed(fn):
    for _ in range(10):
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


res = {"faces": int(len(faces_np)), "vertices": int(len(verts_np)), "calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "cases": {}}
for size in (1024, 2048):
    cam = scenes.orbit_camera(size, size, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    clip = (torch.nn.functional.pad(verts, (0, 1), value=1.0) @ torch.from_numpy(cam.projmatrix).to(dev)).contiguous()[None]
    rast, _ = dr.rasterize(glctx, clip, faces, (size, size))
    covered = int((rast[..., 3] > 0).sum())
    case = {"covered_pixels": covered, "faces_seen": int(dr.face_ids(rast).unique().numel() - 1)}
    case["rasterize"] = timed(lambda: dr.rasterize(glctx, clip, faces, (size, size), validate=False))
    case["rasterize_validate"] = timed(lambda: dr.rasterize(glctx, clip, faces, (size, size)))
    mask = (verts[:, 1:2] > 0).float().contiguous()
    case["interpolate_C1"] = timed(lambda: dr.interpolate(mask[None], rast, faces))
    case["interpolate_C3"] = timed(lambda: dr.interpolate(verts, rast, faces))
    full, _ = dr.rasterize(glctx, pair_pos, pair_faces, (size, size))
    assert bool((full[..., 3] > 0).all())
    case["rasterize_fullscreen_pair"] = timed(lambda: dr.rasterize(glctx, pair_pos, pair_faces, (size, size), validate=False))
    res["cases"][f"{size}x{size}"] = case
print(json.dumps(res))
