"""What the geometry stage's isosurface costs per step (youreditableavatar_amd.marching_tets, csrc/tgs_marching_tets.hip): forward, and forward +
backward, on the Kuhn grids of tests/mt_ref.py -- 64^3, 128^3 and 256^3 cubes (1.6 M, 12.6 M and 100 M tetrahedra) -- each beside the torch op chain
of tests/mt_ref.py run on the same device in float32, which issues the framework ops the geometry stage's own implementation issues (boolean
masks, ``torch.unique(dim=0)``, sizes read back): that op chain is the comparison, there is no earlier native implementation.

`python3 tools/marching_tets_loop.py [calls per block] [rounds] [grid sizes, comma separated]` -- the protocol of tools/mesh_grad_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per
call, with the spread of the blocks beside it.  A record, not a bar.  A backward is run with a fixed random upstream
through `torch.autograd.grad` with respect to pos and sdf, so the time includes the autograd node, the output allocations and the two
read-backs a trainer pays as well.  The 256^3 grid holds 3.2 GB of int64 indices and takes
several GB of host memory to build; pass `64,128` to leave it out."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from tests import mt_ref
from youreditableavatar_amd import build
from youreditableavatar_amd.marching_tets import marching_tets
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128, 256]
dev = torch.device("cuda", 0)


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


res = {"calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "cases": {}}
for n in sizes:
    s = mt_ref.kuhn(n)
    pos, sdf, tet = (torch.from_numpy(s[k].copy()).to(dev) for k in ("pos", "sdf", "tet"))
    tet32 = tet.int()
    pos_g, sdf_g = pos.clone().requires_grad_(True), sdf.clone().requires_grad_(True)
    out = marching_tets(pos, sdf, tet)
    ref = mt_ref.marching_tets(pos, sdf, tet)
    assert all(torch.equal(out[k], ref[k]) for k in mt_ref.KEYS[1:])           # the two produce the same mesh
    g = torch.rand(out["verts"].shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) - 0.5
    case = {"vertices": len(pos), "tetrahedra": len(tet), "valid_tets": int(out["valid_tets"].sum()), "mesh_vertices": len(out["verts"]), "faces": len(out["faces"]),
            "verts_max_abs_diff_to_op_chain": float((out["verts"] - ref["verts"]).abs().max())}

    def step(fn, t):
        torch.autograd.grad(fn(pos_g, sdf_g, t)["verts"], (pos_g, sdf_g), g)
    case["native_forward_int64"] = timed(lambda: marching_tets(pos, sdf, tet))
    case["native_forward_int32"] = timed(lambda: marching_tets(pos, sdf, tet32))
    case["native_forward_backward_int64"] = timed(lambda: step(marching_tets, tet))
    case["op_chain_forward"] = timed(lambda: mt_ref.marching_tets(pos, sdf, tet))
    case["op_chain_forward_backward"] = timed(lambda: step(mt_ref.marching_tets, tet))
    res["cases"][f"kuhn_{n}"] = case
    print(json.dumps({f"kuhn_{n}": case}), flush=True)
    del pos, sdf, tet, tet32, pos_g, sdf_g, out, ref, g
    torch.cuda.empty_cache()
print(json.dumps(res))
