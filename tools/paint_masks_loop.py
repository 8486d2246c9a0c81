"""What the painting stage's masks cost (youreditableavatar_amd.mask_ops, csrc/tgs_mask_ops.hip; youreditableavatar_amd.mesh_region, csrc/tgs_mesh_region.hip),
each next to the torch formulation it replaces:

  images   1024^2 and 2048^2, three channels, uint8: the chain of ``prepare_mask_proj``, erode 2 -> dilate 20 -> float -> blur 21 -> ``> 0``, and its parts;
           in torch: padded ``max_pool2d`` for the rectangle and ``conv2d`` over a reflect-padded image for the blur, in float32
  mesh     an icosphere of 20 * 4^subdivisions faces (8: 1 310 720), the hit faces a cap around +z and a small second cap: ``refine_region`` at (2, 5)
           and (8, 10), in torch ``index_add_`` of the selection onto the vertices and a gather back per iteration; and the components pass,
           ``keep_large_components`` at a quarter of the region, which has no torch formulation beside it

`python3 tools/paint_masks_loop.py [calls per block] [rounds] [subdivisions of the icosphere] [output file]` -- the protocol of tools/mesh_sdf_loop.py: per
case a warm-up of 10 calls, then `rounds` blocks of `calls` calls each between two synchronisations; the figure is the median block's time per call, with
the spread of the blocks beside it.  A record, not a bar: nothing ran on this hardware before, and the reference's host path
(cv2, pymeshlab) is not installed.  The tool asserts equal results of both formulations before it times them."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import torch.nn.functional as F
from youreditableavatar_amd import build, mask_ops as mo, mesh_region as mr, scenes
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
subdiv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
out_path = sys.argv[4] if len(sys.argv) > 4 else None
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


# ---- the torch formulations ----
def torch_morph(img, k, dilate):
    """[H,W,C] uint8 -> the same, through a padded max_pool2d in float32 (exact on 0 .. 255)"""
    a = k // 2
    x = img.permute(2, 0, 1)[None].float()
    x = x if dilate else 255.0 - x
    x = F.max_pool2d(F.pad(x, (a, k - 1 - a, a, k - 1 - a), value=0.0), k, stride=1)
    x = x if dilate else 255.0 - x
    return x[0].permute(1, 2, 0).to(torch.uint8)


def torch_blur(img, k):
    """[H,W,C] float32 -> the same: two conv2d passes over a reflect-padded image, float32 weights and sums"""
    w = torch.from_numpy(mo.gaussian_kernel(k)).float().to(img.device)
    C, r = img.shape[2], k // 2
    x = F.pad(img.permute(2, 0, 1)[None], (r, r, r, r), mode="reflect")
    x = F.conv2d(x, w.view(1, 1, 1, k).expand(C, 1, 1, k), groups=C)
    x = F.conv2d(x, w.view(1, 1, k, 1).expand(C, 1, k, 1), groups=C)
    return x[0].permute(1, 2, 0)


def torch_region(faces64, sel, V, dilate_iter, erode_iter):
    flat = faces64.reshape(-1)
    for _ in range(dilate_iter):
        marked = torch.zeros(V, dtype=torch.int32, device=sel.device).index_add_(0, flat, sel.repeat_interleave(3).int()) > 0
        sel = marked[faces64].any(dim=1)
    for _ in range(erode_iter):
        has_sel = torch.zeros(V, dtype=torch.int32, device=sel.device).index_add_(0, flat, sel.repeat_interleave(3).int()) > 0
        has_unsel = torch.zeros(V, dtype=torch.int32, device=sel.device).index_add_(0, flat, (~sel).repeat_interleave(3).int()) > 0
        sel = (has_sel & ~has_unsel)[faces64].all(dim=1)
    vertex_mask = torch.zeros(V, dtype=torch.int32, device=sel.device).index_add_(0, flat, sel.repeat_interleave(3).int()) > 0
    return sel, vertex_mask


res = {"calls_per_block": calls, "rounds": rounds, "library": build.source_hash(), "cases": {}}
ones = lambda k: np.ones((k, k), np.uint8)
for size in (1024, 2048):
    yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
    gen = torch.Generator(device=dev).manual_seed(size)
    blobs = ((yy - size * 0.4) ** 2 + (xx - size * 0.55) ** 2 < (size * 0.17) ** 2) | (torch.rand((size, size), device=dev, generator=gen) < 0.0005)
    mask = (blobs[:, :, None].expand(size, size, 3) * 255).to(torch.uint8).contiguous()

    ours = lambda: mo.gaussian_blur(mo.dilate(mo.erode(mask, ones(2)), ones(20)).float(), (21, 21), 0) > 0
    theirs = lambda: torch_blur(torch_morph(torch_morph(mask, 2, False), 20, True).float(), 21) > 0
    assert torch.equal(mo.erode(mask, 2), torch_morph(mask, 2, False)) and torch.equal(mo.dilate(mask, 20), torch_morph(mask, 20, True)) and torch.equal(mo.dilate(mask, 5), torch_morph(mask, 5, True))
    assert torch.equal(ours(), theirs())
    dil = mo.dilate(mask, 20).float()
    rel = ((mo.gaussian_blur(dil, (21, 21)) - torch_blur(dil, 21)).abs() / 255.0).max()
    case = {"pixels": size * size, "channels": 3, "set_share": round(float(blobs.float().mean()), 4), "blur_max_abs_diff_to_torch_fp32_over_255": float(rel),
            "chain": timed(ours), "chain_torch": timed(theirs),
            "erode_2": timed(lambda: mo.erode(mask, 2)), "erode_2_torch": timed(lambda: torch_morph(mask, 2, False)),
            "dilate_20": timed(lambda: mo.dilate(mask, 20)), "dilate_20_torch": timed(lambda: torch_morph(mask, 20, True)),
            "dilate_5": timed(lambda: mo.dilate(mask, 5)), "dilate_5_torch": timed(lambda: torch_morph(mask, 5, True)),
            "blur_21": timed(lambda: mo.gaussian_blur(dil, (21, 21))), "blur_21_torch": timed(lambda: torch_blur(dil, 21))}
    case["chain_speedup"] = round(case["chain_torch"]["median_ms"] / case["chain"]["median_ms"], 2)
    res["cases"][f"image_{size}"] = case
    print(json.dumps({f"image_{size}": case}), flush=True)
    del yy, xx, blobs, mask, dil

v, f = scenes.icosphere(subdiv)
V, nF = len(v), len(f)
centroid = v[f.astype(np.int64)].mean(axis=1)
hit_np = (centroid[:, 2] > 0.8) | ((centroid[:, 0] > 0.995) & (centroid[:, 2] < 0.05))           # a cap around +z and a small one around +x
faces = torch.from_numpy(f.astype(np.int32)).to(dev)
faces64 = faces.long()
hit = torch.from_numpy(hit_np).to(dev)
case = {"vertices": V, "faces": nF, "hit_faces": int(hit_np.sum())}
for d, e in ((2, 5), (8, 10)):
    region = mr.refine_region(faces, hit, V, d, e)
    want_f, want_v = torch_region(faces64, hit, V, d, e)
    assert torch.equal(region.face_mask, want_f) and torch.equal(region.vertex_mask, want_v)
    case[f"refine_region_{d}_{e}"] = timed(lambda: mr.refine_region(faces, hit, V, d, e))
    case[f"refine_region_{d}_{e}_torch"] = timed(lambda: torch_region(faces64, hit, V, d, e))
    case[f"refine_region_{d}_{e}_faces"] = int(region.face_mask.sum())
    case[f"refine_region_{d}_{e}_speedup"] = round(case[f"refine_region_{d}_{e}_torch"]["median_ms"] / case[f"refine_region_{d}_{e}"]["median_ms"], 2)
region = mr.refine_region(faces, hit, V, 8, 10)
label, size = mr.face_components(region.face_mask, faces, V)
n_region = int(region.face_mask.sum())
kept = mr.keep_large_components(region.face_mask, faces, V, int(n_region * 0.25))
case["components"] = {"region_faces": n_region, "components": int(torch.unique(label[label >= 0]).numel()), "kept_faces": int(kept.sum()), "rounds": mr.last_component_rounds,
                      "cap_rounds": nF + 16, "readbacks": mr.last_component_rounds // mr.ROUNDS_PER_READBACK}
case["keep_large_components"] = timed(lambda: mr.keep_large_components(region.face_mask, faces, V, int(n_region * 0.25)), warm=3)
full = torch.ones(nF, dtype=torch.bool, device=dev)
label, size = mr.face_components(full, faces, V)
assert int(label.max()) == 0 and int(size.min()) == nF                          # the whole sphere is one component
case["components_whole_mesh"] = {"rounds": mr.last_component_rounds, "readbacks": mr.last_component_rounds // mr.ROUNDS_PER_READBACK}
case["face_components_whole_mesh"] = timed(lambda: mr.face_components(full, faces, V), warm=3)
res["cases"][f"icosphere_{subdiv}"] = case
print(json.dumps({f"icosphere_{subdiv}": case}), flush=True)
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
