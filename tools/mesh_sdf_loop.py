"""What the shape initialisation's target costs (youreditableavatar_amd.mesh_sdf, csrc/tgs_mesh_sdf.hip): the signed distance of 40 000 uniform points
in [-1, 1]^3 -- what one iteration of ``ImplicitSDF.initialize_shape`` draws -- to the body mesh of tests/golden/ref_mesh_sdf_fixture.npz (20 908 faces)
through the tree (mode 0) and over every face (mode 1), to the icosphere of tools/mesh_raster_loop.py scaled to 0.9 (1 310 720 faces) through the tree,
one whole iteration of the initialisation (the points, ``SDF``, ``SdfField`` forward and backward with the reference's default config, Adam) with the
query's share of it, and the host build of both trees.  There is no earlier implementation on this hardware and pysdf is not installed: nothing stands
beside these figures.

`python3 tools/mesh_sdf_loop.py [calls per block] [rounds] [subdivisions of the icosphere] [output file]` -- the protocol of tools/mesh_geom_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with
the spread of the blocks beside it.  The host builds are timed one by one (3 builds, the median).  A record, not a bar.  The tool
asserts that mode 0 and mode 1 give the same bits on the body mesh before it times them."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from tests import hashgrid_ref, mesh_sdf_ref
from youreditableavatar_amd import build, hashgrid as hg, scenes
from youreditableavatar_amd.mesh_sdf import SDF
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
subdiv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
out_path = sys.argv[4] if len(sys.argv) > 4 else None
N = 40000
dev = torch.device("cuda", 0)


def timed(fn, warm=10):
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


def host_build(v, f):
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        sdf = SDF(v, f)
        ms.append((time.perf_counter() - t0) * 1e3)
    return sdf, {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2), "tree_MB": round(sdf._bytes / 2 ** 20, 1)}


res = {"calls_per_block": calls, "rounds": rounds, "points": N, "library": build.source_hash(), "cases": {}}
gen = torch.Generator(device=dev).manual_seed(3)
points = torch.rand((N, 3), device=dev, generator=gen) * 2.0 - 1.0
body_v, body_f = mesh_sdf_ref.load_fixture()[:2]
body, t_body = host_build(body_v, body_f)
a, b = body.closest(points, mode=0), body.closest(points, mode=1)
assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)) and torch.equal(body.contains(points, mode=0), body.contains(points, mode=1))
case = {"vertices": len(body_v), "faces": len(body_f), "host_build_with_upload": t_body, "inside_share": round(float(body.contains(points).float().mean()), 4)}
case["query_tree"] = timed(lambda: body(points))
case["query_tree_sdf_face_closest"] = timed(lambda: body.closest(points))
case["query_every_face"] = timed(lambda: body(points, mode=1), warm=2)
res["cases"]["body"] = case
print(json.dumps({"body": case}), flush=True)

# one iteration of the shape initialisation: the points, the target, the field forward and backward, Adam (lr 1e-3, as the reference sets it)
config = hashgrid_ref.CONFIGS["default"]
encoding = hg.HashGrid(3, config)
mlp = torch.nn.Sequential(torch.nn.Linear(encoding.n_output_dims, 64, bias=False), torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 1, bias=False))
field = hg.SdfField(encoding, mlp, bbox=[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], bias=0.0).to(dev)
opt = torch.optim.Adam(field.parameters(), lr=1e-3)


def iteration(target_of):
    p = torch.rand((N, 3), device=dev) * 2.0 - 1.0
    loss = torch.nn.functional.mse_loss(field(p), target_of(p))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()


step = {"iteration": timed(lambda: iteration(lambda p: -body(p)[..., None])),
        "iteration_with_a_constant_target": timed(lambda: iteration(lambda p: p[:, :1])),
        "iteration_through_the_host_as_the_reference_writes_it": timed(lambda: iteration(lambda p: torch.from_numpy(-body(p.cpu().numpy())).to(p)[..., None]))}
step["query_share_of_iteration"] = round(case["query_tree"]["median_ms"] / step["iteration"]["median_ms"], 3)
res["cases"]["stage0_iteration_body"] = step
print(json.dumps({"stage0_iteration_body": step}), flush=True)

ico_v, ico_f = scenes.icosphere(subdiv)
ico_v = (ico_v * np.float32(0.9)).astype(np.float32)
ico, t_ico = host_build(ico_v, ico_f)
case = {"vertices": len(ico_v), "faces": len(ico_f), "host_build_with_upload": t_ico, "inside_share": round(float(ico.contains(points).float().mean()), 4),
        "sphere_volume_share": round(4.0 / 3.0 * np.pi * 0.9 ** 3 / 8.0, 4)}
d = ico(points)
case["max_abs_diff_to_the_sphere"] = float((d - (0.9 - points.norm(dim=1))).abs().max())
case["query_tree"] = timed(lambda: ico(points))
res["cases"][f"icosphere_{subdiv}"] = case
print(json.dumps({f"icosphere_{subdiv}": case}), flush=True)
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
