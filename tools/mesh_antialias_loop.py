"""What `antialias` costs (youreditableavatar_amd.mesh_raster_aa, csrc/tgs_mesh_aa.hip): the sphere of tools/mesh_raster_loop.py (1 310 720 faces) through
its orbit camera at 1024 x 1024 and 2048 x 2048, a vertex mask (C = 1) and the normals (C = 3), with a prebuilt topology and with the topology
built in the call, the topology build on its own, and -- for context, in the same run -- `rasterize` and `interpolate`.

`python3 tools/mesh_antialias_loop.py [calls per block] [rounds] [subdivisions]` -- the protocol of tools/mesh_raster_loop.py: per case a warm-up of
10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with the
spread of the blocks beside it.  There is no earlier implementation on this hardware: a record, not a bar.  `bytes_min` is
what a call must move at the least: 16 B of rast and 8 C B of colour in and out per pixel; the per-pair reads (12 B of tri, 48 B of pos, 4 B of
topo per analysed pair, mostly cache hits) are counted beside it as `pair_bytes`."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import youreditableavatar_amd.mesh_raster_aa as dr
from youreditableavatar_amd import build, scenes
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
subdiv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
dev = torch.device("cuda", 0)
verts_np, faces_np = scenes.icosphere(subdiv)
verts, faces = torch.from_numpy(verts_np).to(dev), torch.from_numpy(faces_np).to(dev)
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
res["topology_build"] = timed(lambda: dr.antialias_construct_topology_hash(faces))
topo = dr.antialias_construct_topology_hash(faces)
res["topology_open_edges"] = int((topo == -1).sum())
res["topology_workspace_bytes"] = int(dr._lib.tgs_mesh_topology_workspace_bytes(len(faces_np)))
for size in (1024, 2048):
    cam = scenes.orbit_camera(size, size, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    clip = (torch.nn.functional.pad(verts, (0, 1), value=1.0) @ torch.from_numpy(cam.projmatrix).to(dev)).contiguous()[None]
    rast, _ = dr.rasterize(glctx, clip, faces, (size, size))
    ids = dr.face_ids(rast)[0]
    pairs = int((ids[:, 1:] != ids[:, :-1]).sum() + (ids[1:] != ids[:-1]).sum())
    case = {"covered_pixels": int((ids >= 0).sum()), "pairs_analysed": pairs, "pair_bytes": pairs * 64}
    case["rasterize"] = timed(lambda: dr.rasterize(glctx, clip, faces, (size, size), validate=False))
    vmask = (verts[:, 1:2] > 0).float().contiguous()
    case["interpolate_C1"] = timed(lambda: dr.interpolate(vmask[None], rast, faces))
    case["interpolate_C3"] = timed(lambda: dr.interpolate(verts, rast, faces))
    for C, attr in ((1, vmask), (3, verts)):
        color, _ = dr.interpolate(attr, rast, faces)
        out = dr.antialias(color, rast, clip, faces, topology_hash=topo)
        case[f"antialias_C{C}_blended_pixels"] = int((out != color).any(dim=-1).sum())
        case[f"antialias_C{C}_bytes_min"] = size * size * (16 + 8 * C)
        case[f"antialias_C{C}"] = timed(lambda: dr.antialias(color, rast, clip, faces, topology_hash=topo))
        case[f"antialias_C{C}_with_topology_build"] = timed(lambda: dr.antialias(color, rast, clip, faces))
    res["cases"][f"{size}x{size}"] = case
print(json.dumps(res))
