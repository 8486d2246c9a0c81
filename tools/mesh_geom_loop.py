"""What the geometry stage's mesh normals and smoothness losses cost per step (youreditableavatar_amd.mesh_geom, csrc/tgs_mesh_geom.hip) on the
meshes that marching_tets makes of the Kuhn grids of tests/mt_ref.py -- 64^3, 128^3 and 256^3 cubes, the sizes of INTEGRATION.md 4m -- each beside the
torch op chain of tests/mesh_geom_ref.py run on the same device in float32, which issues framework ops of the kind the geometry stage's own
implementation issues (gathers, ``index_add_`` with float atomics, ``torch.unique(dim=0)``): that op chain is the comparison, there is no earlier
native implementation.

`python3 tools/mesh_geom_loop.py [calls per block] [rounds] [grid sizes, comma separated]` -- the protocol of tools/marching_tets_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per
call, with the spread of the blocks beside it.  A record, not a bar.  Timed: the topology (with its read-back); the normals
forward and forward + backward on a topology built before; the step's set -- on a fresh mesh the topology, two normal calls, the consistency
of the first one's normals, and the backward of all three with fixed upstreams -- against the op chain's set: two normal calls, the edges, the
consistency, the backward.  The Laplacian is timed beside them.  The 256^3 grid takes several GB of host memory to build; pass `64,128` to
leave it out."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from tests import mesh_geom_ref as ref
from tests import mt_ref
from youreditableavatar_amd import build, mesh_geom as mg
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
    with torch.no_grad():
        mesh = marching_tets(*(torch.from_numpy(s[k].copy()).to(dev) for k in ("pos", "sdf", "tet")))
    v, f = mesh["verts"].clone(), mesh["faces"].clone()
    del mesh, s
    torch.cuda.empty_cache()
    V = len(v)
    vg = v.clone().requires_grad_(True)
    topo = mg.mesh_topology(f, V)
    edges = ref.edges_of(f)
    assert torch.equal(topo.edges, edges)                                       # the two find the same edges
    gen = torch.Generator(device=dev).manual_seed(3)
    g1, g2 = (torch.rand((V, 3), device=dev, generator=gen) - 0.5 for _ in range(2))
    n_native, n_chain = mg.vertex_normals(v, f, topo), ref.vertex_normals(v, f)
    case = {"vertices": V, "faces": len(f), "edges": topo.num_edges, "normals_max_abs_diff_to_op_chain": float((n_native - n_chain).abs().max()),
            "consistency": [float(mg.normal_consistency(n_native, topo)), float(ref.normal_consistency(n_chain, edges))],
            "laplacian": [float(mg.laplacian(v, topo)), float(ref.laplacian(v, edges))]}

    def native_set():
        t = mg.mesh_topology(f, V)
        a, b = mg.vertex_normals(vg, f, t), mg.vertex_normals(vg, f, t)
        torch.autograd.grad((a * g1).sum() + (b * g2).sum() + 2000.0 * mg.normal_consistency(a, t), vg)

    def chain_set():
        a, b = ref.vertex_normals(vg, f), ref.vertex_normals(vg, f)
        torch.autograd.grad((a * g1).sum() + (b * g2).sum() + 2000.0 * ref.normal_consistency(a, ref.edges_of(f)), vg)
    case["native_topology"] = timed(lambda: mg.mesh_topology(f, V))
    case["native_topology_no_edges"] = timed(lambda: mg.mesh_topology(f, V, edges=False))
    case["op_chain_edges"] = timed(lambda: ref.edges_of(f))
    case["native_normals_forward"] = timed(lambda: mg.vertex_normals(v, f, topo))
    case["native_normals_forward_backward"] = timed(lambda: torch.autograd.grad(mg.vertex_normals(vg, f, topo), vg, g1))
    case["op_chain_normals_forward"] = timed(lambda: ref.vertex_normals(v, f))
    case["op_chain_normals_forward_backward"] = timed(lambda: torch.autograd.grad(ref.vertex_normals(vg, f), vg, g1))
    case["native_laplacian_forward_backward"] = timed(lambda: torch.autograd.grad(mg.laplacian(vg, topo), vg))
    case["op_chain_laplacian_forward_backward"] = timed(lambda: torch.autograd.grad(ref.laplacian(vg, edges), vg))
    case["native_step_set"] = timed(native_set)
    case["op_chain_step_set"] = timed(chain_set)
    res["cases"][f"kuhn_{n}"] = case
    print(json.dumps({f"kuhn_{n}": case}), flush=True)
    del v, f, vg, topo, edges, g1, g2, n_native, n_chain
    torch.cuda.empty_cache()
print(json.dumps(res))
