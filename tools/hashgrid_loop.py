"""What the geometry stage's SDF field costs per call (youreditableavatar_amd.hashgrid, csrc/tgs_hashgrid.hip) on the vertices of the Kuhn grids of
tests/mt_ref.py -- 64^3, 128^3 and 256^3 cubes -- with the reference's default config (16 levels x 2 features, 2^19 entries, 64 neurons, one output),
each beside the torch op chain of tests/hashgrid_ref.py run on the same device in float32, which issues framework ops of the kind a substitute for
tiny-cuda-nn would issue (gathers, ``index_put_`` with float atomics in the backward, two matmuls with their activations kept): that op chain is the
comparison, there is no earlier native implementation and no published number.

`python3 tools/hashgrid_loop.py [calls per block] [rounds] [grid sizes, comma separated] [output file]` -- the protocol of tools/mesh_geom_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with
the spread of the blocks beside it, and ``torch.cuda.max_memory_allocated`` over the case's calls above what was allocated before them.  A record
(INTEGRATION.md 4o), not a bar.  Timed: the encoding forward and forward + backward (dL_dparams), the fused field forward and forward + backward
(dL_dparams, dL_dW1, dL_dW2).  Beside each native figure stands what the gather alone would cost: 16 levels x 8 corners x 8 bytes per point, at
the rates given in the environment (HBM_GBS, L2_GBS; the defaults, 4 and 14 TB/s, are round figures below what kilobyte rows gathered from HBM and
from an XCD's L2 reach on the MI355X, about 6 and 17 TB/s: an 8-byte row fetches a whole cache line, so the useful rate of this gather is lower still)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from tests import hashgrid_ref as ref
from tests import mt_ref
from youreditableavatar_amd import build, hashgrid as hg
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 128, 256]
out_path = sys.argv[4] if len(sys.argv) > 4 else None
HBM_GBS, L2_GBS = float(os.environ.get("HBM_GBS", 4000.0)), float(os.environ.get("L2_GBS", 14000.0))
dev = torch.device("cuda", 0)
config = ref.CONFIGS["default"]
levels, ref_levels = hg.level_table(config), ref.level_table(config)


def timed(fn):
    try:
        return _timed(fn)
    except RuntimeError as e:                          # (the op chain at 256^3: the framework's index_put sorts more than 2^31 elements and refuses)
        torch.cuda.empty_cache()
        return {"failed": str(e).splitlines()[0][:160]}


def _timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / calls * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "peak_extra_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)}


gen = torch.Generator(device=dev).manual_seed(3)
P = ((torch.rand(2 * ref.n_entries(ref_levels), device=dev, generator=gen) - 0.5) * 2e-4).requires_grad_(True)
W1 = ((torch.rand((64, 32), device=dev, generator=gen) - 0.5) / 4).requires_grad_(True)
W2 = ((torch.rand((1, 64), device=dev, generator=gen) - 0.5) / 4).requires_grad_(True)
res = {"calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "config": config, "hbm_GBs": HBM_GBS, "l2_GBs": L2_GBS, "cases": {}}
for n in sizes:
    g = np.stack(np.meshgrid(*(np.arange(n + 1),) * 3, indexing="ij"), -1).reshape(-1, 3) / n if n > 128 else None
    # (the 256^3 grid's tetrahedra take several GB of host memory to build and are not needed here: its vertices are the same lattice, unjittered)
    x = torch.from_numpy(g.astype(np.float32) if g is not None else mt_ref.kuhn(n)["pos"].copy()).to(dev).clamp_(0.0, 1.0)
    N = len(x)
    g_enc, g_out = torch.rand((N, 32), device=dev, generator=gen) - 0.5, torch.rand((N, 1), device=dev, generator=gen) - 0.5
    gather_bytes = N * len(levels) * 8 * 8
    case = {"points": N, "gather_MB": round(gather_bytes / 2 ** 20, 1), "gather_at_hbm_ms": round(gather_bytes / HBM_GBS / 1e6, 4),
            "gather_at_l2_ms": round(gather_bytes / L2_GBS / 1e6, 4)}
    with torch.no_grad():
        a, b = hg.hashgrid_encode(x, P, levels), ref.encode(x, P.detach(), ref_levels)[0]
        case["encode_max_abs_diff_to_op_chain"] = float((a - b).abs().max())
        a, b = hg.sdf_field(x, P, levels, W1, W2, bias=0.1), ref.field(x, P.detach(), ref_levels, W1.detach(), W2.detach(), None, 0.1)[0]
        case["field_max_abs_diff_to_op_chain"] = float((a - b).abs().max())
        del a, b
        case["native_encode_forward"] = timed(lambda: hg.hashgrid_encode(x, P, levels))
        case["op_chain_encode_forward"] = timed(lambda: ref.encode(x, P, ref_levels)[0])
        case["native_field_forward"] = timed(lambda: hg.sdf_field(x, P, levels, W1, W2, bias=0.1))
        case["op_chain_field_forward"] = timed(lambda: ref.field(x, P, ref_levels, W1, W2, None, 0.1)[0])
    case["native_encode_forward_backward"] = timed(lambda: torch.autograd.grad(hg.hashgrid_encode(x, P, levels), P, g_enc))
    case["op_chain_encode_forward_backward"] = timed(lambda: torch.autograd.grad(ref.encode(x, P, ref_levels)[0], P, g_enc))
    case["native_field_forward_backward"] = timed(lambda: torch.autograd.grad(hg.sdf_field(x, P, levels, W1, W2, bias=0.1), (P, W1, W2), g_out))
    case["op_chain_field_forward_backward"] = timed(lambda: torch.autograd.grad(ref.field(x, P, ref_levels, W1, W2, None, 0.1)[0], (P, W1, W2), g_out))
    res["cases"][f"kuhn_{n}"] = case
    print(json.dumps({f"kuhn_{n}": case}), flush=True)
    del x, g_enc, g_out
    torch.cuda.empty_cache()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
