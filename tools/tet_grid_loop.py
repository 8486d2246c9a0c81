"""What the geometry stage's grid passes cost per step (youreditableavatar_amd.tet_grid, csrc/tgs_tet_grid.hip): `compact_tets` on the Kuhn
grids of tests/mt_ref.py -- 64^3 and 128^3 cubes (1.6 M and 12.6 M tetrahedra) -- then `subdivide_tets` of its result, each beside the torch op
chain of tests/tet_ref.py run on the same device, which issues the framework ops the geometry stage's own implementation issues (boolean masks,
``torch.unique(..., return_inverse=True)``, stacks and a cat): that op chain is the comparison, there is no earlier native implementation.

`python3 tools/tet_grid_loop.py [calls per block] [rounds] [grid sizes, comma separated]` -- the protocol of tools/marching_tets_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per
call, with the spread of the blocks beside it.  A record, not a bar.  The tool asserts that the native call and the op chain
give equal outputs, element for element and bit for bit, before it times them.  The times include the wrappers: the read-back, the output
allocations and the workspace.  The defaults keep one run under a minute."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from tests import mt_ref, tet_ref
from youreditableavatar_amd import build
from youreditableavatar_amd.tet_grid import compact_tets, subdivide_tets
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128]
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


def same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape == w.shape and torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g.long(), w.view(torch.int32) if w.dtype == torch.float32 else w.long())


res = {"calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "cases": {}}
for n in sizes:
    s = mt_ref.kuhn(n)
    pos, sdf, tet = (torch.from_numpy(s[k].copy()).to(dev) for k in ("pos", "sdf", "tet"))
    sdf = sdf[:, None]
    mask = (pos[:, :1] < 0.5).int()
    tet32 = tet.int()
    c = compact_tets(pos, sdf, tet, mask)
    d = subdivide_tets(c[0], c[2], c[3])
    same(c, tet_ref.compact_tets(pos, sdf, tet, mask))                          # the two produce the same grids
    same(d, tet_ref.subdivide_tets(c[0], c[2], c[3]))
    case = {"vertices": len(pos), "tetrahedra": len(tet), "kept_tetrahedra": len(c[4]), "kept_vertices": len(c[0]), "edges": len(d[4]), "sub_tetrahedra": len(d[1])}
    case["native_compact_int64"] = timed(lambda: compact_tets(pos, sdf, tet, mask))
    case["native_compact_int32"] = timed(lambda: compact_tets(pos, sdf, tet32, mask))
    case["native_subdivide"] = timed(lambda: subdivide_tets(c[0], c[2], c[3]))
    case["native_compact_then_subdivide"] = timed(lambda: subdivide_tets(*(lambda r: (r[0], r[2], r[3]))(compact_tets(pos, sdf, tet, mask))))
    case["op_chain_compact"] = timed(lambda: tet_ref.compact_tets(pos, sdf, tet, mask))
    case["op_chain_subdivide"] = timed(lambda: tet_ref.subdivide_tets(c[0], c[2], c[3]))
    case["op_chain_compact_then_subdivide"] = timed(lambda: tet_ref.subdivide_tets(*(lambda r: (r[0], r[2], r[3]))(tet_ref.compact_tets(pos, sdf, tet, mask))))
    res["cases"][f"kuhn_{n}"] = case
    print(json.dumps({f"kuhn_{n}": case}), flush=True)
    del pos, sdf, tet, tet32, mask, c, d
    torch.cuda.empty_cache()
print(json.dumps(res))
