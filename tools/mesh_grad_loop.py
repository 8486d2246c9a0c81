"""What a training step costs on the mesh rasterizer (youreditableavatar_amd.mesh_raster_grad, csrc/tgs_mesh_grad.hip): forward + backward of
`rasterize`, `interpolate` and `antialias` on the sphere of tools/mesh_raster_loop.py (1 310 720 faces) through its orbit camera at 1024 x 1024
and 2048 x 2048, the normals (C = 3) and a vertex mask (C = 1), each beside its forward alone.

`python3 tools/mesh_grad_loop.py [calls per block] [rounds] [subdivisions]` -- the protocol of tools/mesh_raster_loop.py: per case a warm-up of
10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with the
spread of the blocks beside it.  There is no earlier implementation on this hardware: a record, not a bar.  A backward is
run with a fixed random upstream through `torch.autograd.grad`, so the time includes the autograd node and the output allocations a trainer
pays as well."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import youreditableavatar_amd.mesh_raster_grad as dr
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
topo = dr.antialias_construct_topology_hash(faces)
gen = torch.Generator(device=dev).manual_seed(3)
for size in (1024, 2048):
    cam = scenes.orbit_camera(size, size, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    clip = (torch.nn.functional.pad(verts, (0, 1), value=1.0) @ torch.from_numpy(cam.projmatrix).to(dev)).contiguous()
    clip_g = clip.clone().requires_grad_(True)
    rast, _ = dr.rasterize(glctx, clip[None], faces, (size, size))
    case = {"covered_pixels": int((dr.face_ids(rast) >= 0).sum())}
    g4 = torch.rand((1, size, size, 4), device=dev, generator=gen) - 0.5

    def rasterize_step():
        r, _ = dr.rasterize(glctx, clip_g[None], faces, (size, size), validate=False)
        torch.autograd.grad(r, clip_g, g4)
    case["rasterize_forward"] = timed(lambda: dr.rasterize(glctx, clip[None], faces, (size, size), validate=False))
    case["rasterize_forward_backward"] = timed(rasterize_step)
    for C, attr in ((1, (verts[:, 1:2] > 0).float().contiguous()), (3, verts)):
        attr_g, rast_g = attr.clone().requires_grad_(True), rast.clone().requires_grad_(True)
        g = torch.rand((1, size, size, C), device=dev, generator=gen) - 0.5
        color, _ = dr.interpolate(attr, rast, faces)
        color_g = color.clone().requires_grad_(True)

        def interpolate_step(wrt):
            out, _ = dr.interpolate(attr_g, rast_g if len(wrt) == 2 else rast, faces)
            torch.autograd.grad(out, wrt, g)

        def antialias_step(with_color):
            out = dr.antialias(color_g if with_color else color, rast, clip_g, faces, topology_hash=topo)
            torch.autograd.grad(out, (color_g, clip_g) if with_color else (clip_g,), g)
        case[f"interpolate_C{C}_forward"] = timed(lambda: dr.interpolate(attr, rast, faces))
        case[f"interpolate_C{C}_forward_backward_attr"] = timed(lambda: interpolate_step((attr_g,)))
        case[f"interpolate_C{C}_forward_backward_attr_rast"] = timed(lambda: interpolate_step((attr_g, rast_g)))
        case[f"antialias_C{C}_forward"] = timed(lambda: dr.antialias(color, rast, clip, faces, topology_hash=topo))
        case[f"antialias_C{C}_forward_backward_pos"] = timed(lambda: antialias_step(False))
        case[f"antialias_C{C}_forward_backward_color_pos"] = timed(lambda: antialias_step(True))
    res["cases"][f"{size}x{size}"] = case
print(json.dumps(res))
