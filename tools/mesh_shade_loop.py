"""What an optimisation step of the geometry stage costs on its renderer body (youreditableavatar_amd.mesh_shade, csrc/tgs_mesh_shade.hip): forward +
backward of `mesh_shade.render` itself on the sphere of tools/mesh_raster_loop.py through its orbit camera at 512 x 512 and 1024 x 1024, beside the
unfused body the reference's lines (models/renderers/part_nvdiff_rasterizer.py :100-152) make out of `mesh_raster_grad`, `mesh_geom` and the
framework's calls, in the same process.

`python3 tools/mesh_shade_loop.py [calls per block] [rounds] [subdivisions]` -- the protocol of tools/mesh_grad_loop.py: per case a warm-up of 10
calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with the spread of
the blocks beside it.  Both paths start from the vertices and the camera matrices (the transform and the vertex normals are inside the timed
call), take the two topologies of the mesh as given (built once per mesh), do not validate the indices, and differentiate a fixed random upstream
with respect to the vertices.  `launches` counts the device activities of one forward + backward call (kernels, memsets, copies) with the
framework's profiler; `host_syncs` counts the warnings of the framework's synchronisation check (`torch.cuda.set_sync_debug_mode("warn")`) over
one forward + backward call."""
import json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import youreditableavatar_amd.mesh_raster_grad as dr
import youreditableavatar_amd.mesh_shade as ms
from youreditableavatar_amd import build, mesh_geom, scenes
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
    ms_ = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms_.append((time.perf_counter() - t0) / calls * 1e3)
    return {"median_ms": round(statistics.median(ms_), 4), "min_ms": round(min(ms_), 4), "max_ms": round(max(ms_), 4)}


def launches(fn):
    """device activities of one call, after a warm call"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)


def host_syncs(fn):
    """calls of one fn() that wait for the device, as the framework's synchronisation check reports them"""
    fn()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for w in seen if "synchroniz" in str(w.message))


def unfused(v, mvp, c2w, topo, inc, size):
    """the reference's lines over this package's calls: three antialias calls, two interpolate calls, and the framework calls between them"""
    pos = torch.matmul(torch.nn.functional.pad(v, (0, 1), value=1.0), mvp.permute(0, 2, 1)).contiguous()
    rast, _ = dr.rasterize(glctx, pos, faces, (size, size), validate=False)
    mask = rast[..., 3:] > 0
    opacity = dr.antialias(mask.float(), rast, pos, faces, topology_hash=topo)
    gb, _ = dr.interpolate(mesh_geom.vertex_normals(v, faces, inc), rast, faces)
    gb = torch.matmul(torch.linalg.inv(c2w[:, :3, :3]), gb.view(-1, size * size, 3)[0][:, :, None])
    gb = torch.where(gb[:, 2:3] < 0, -gb, gb).view(-1, size, size, 3)
    gb = torch.nn.functional.normalize(gb, dim=-1)
    normal = dr.antialias(torch.lerp(torch.zeros_like(gb), (gb + 1.0) / 2.0, mask.float()), rast, pos, faces, topology_hash=topo)
    gd, _ = dr.interpolate(pos[0, :, :3].contiguous(), rast, faces)
    gd = 1.0 / (gd[..., 2:3] + 1e-7)
    hi, lo = torch.max(gd[mask[..., 0]]), torch.min(gd[mask[..., 0]])
    depth = dr.antialias(torch.lerp(torch.zeros_like(gd), (gd - lo) / (hi - lo + 1e-7), mask.float()), rast, pos, faces, topology_hash=topo)
    return opacity, normal, depth


def fused(v, mvp, c2w, topo, inc, size):
    """`mesh_shade.render`, as INTEGRATION.md 4t puts it into the renderer, with the two topologies of the mesh"""
    out = ms.render(glctx, v, faces, mvp, (size, size), normal_type="camera", c2w=c2w, topology_hash=topo, normals_topology=inc)
    return out["opacity"], out["comp_normal"], out["comp_depth"]


res = {"faces": int(len(faces_np)), "vertices": int(len(verts_np)), "calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "cases": {}}
topo = dr.antialias_construct_topology_hash(faces)
inc = mesh_geom.mesh_topology(faces, len(verts_np), edges=False)
gen = torch.Generator(device=dev).manual_seed(3)
for size in (512, 1024):
    cam = scenes.orbit_camera(size, size, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    mvp = torch.from_numpy(cam.projmatrix).to(dev).t().contiguous()[None]      # pos_clip = [verts, 1] @ mvp^T
    c2w = torch.eye(4, device=dev)[None].contiguous()
    c2w[0, :3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(5)))[0].to(dev)
    ups = [torch.rand((1, size, size, c), device=dev, generator=gen) - 0.5 for c in (1, 3, 1)]
    verts_g = verts.clone().requires_grad_(True)

    def step(path):
        torch.autograd.grad(path(verts_g, mvp, c2w, topo, inc, size), (verts_g,), ups)
    with torch.no_grad():
        mask = ms.render(glctx, verts, faces, mvp, (size, size), c2w=c2w, topology_hash=topo, normals_topology=inc)["mask"]
    case = {"covered_pixels": int(mask.sum())}
    for name, path in (("unfused", unfused), ("fused", fused)):
        with torch.no_grad():
            case[f"{name}_forward"] = timed(lambda: path(verts, mvp, c2w, topo, inc, size))
        case[f"{name}_forward_backward"] = timed(lambda: step(path))
        case[f"{name}_launches_forward_backward"] = launches(lambda: step(path))
        case[f"{name}_host_syncs_forward_backward"] = host_syncs(lambda: step(path))
    res["cases"][f"{size}x{size}"] = case
print(json.dumps(res))
