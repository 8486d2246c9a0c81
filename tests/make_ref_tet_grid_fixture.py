#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Records what the reference's OWN ``MarchingTetrahedraHelper.compact_tets``, ``.batch_subdivide_volume`` and
``.mark_part_tets`` (Edit_core/tetgs_spatial/models/isosurface.py :208-345) return in float32 on the CPU for the scenes ``odd`` and ``kuhn_8`` of
tests/tet_ref.py, with and without the vertex mask, into tests/golden/ref_tet_grid_fixture.npz: the inputs and every output.  The class is
loaded by tests/make_ref_mt_fixture.py's loader.  The fixture is data: inputs and expected outputs.

Per scene: ``compact`` (sdf as [N,1]) and ``compact_mask``; ``subdiv`` / ``subdiv_mask``: the subdivision of the WHOLE scene; ``chain`` /
``chain_mask``: the subdivision of the compacted scene; ``mark``: mark_part_tets with an ``edit_mask`` (recorded) that marks the faces whose
centroid lies in the half-space x > 1/2.

Asserts that no tetrahedron's |mean sdf| evaluated in float64 lies within 1e-7 of the threshold, apart from the exact rows of ``odd``, so the
fixture does not hang on a summation order; prints the counts."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import make_ref_mt_fixture as M  # noqa: E402
from tests import tet_ref as T  # noqa: E402


def _put(rec, prefix, keys, values):
    for k, v in zip(keys, values):
        if v is not None:
            rec[f"{prefix}.{k}"] = v.numpy()


def main():
    helper = M._instance(M._load_helper())
    rec = {}
    for name in T.FIXTURE_SCENES:
        s = T.scene(name)
        pos, sdf, tet, mask = T.tensors(name)
        for k in ("pos", "sdf", "tet", "mask"):
            rec[f"{name}.{k}"] = s[k]
        mean64 = np.abs(s["sdf"].astype(np.float64)[s["tet"]].mean(1))
        gap = np.abs(mean64 - 0.02)
        free = np.ones(len(gap), bool)
        if name == "odd":
            free[list(T.ODD_EXACT_ROWS)] = False
        free &= np.isfinite(mean64)
        assert gap[free].min() > 1e-7, (name, gap[free].min())
        for tag, m in (("", None), ("_mask", mask)):
            c = helper.compact_tets(pos, sdf, tet, m)
            _put(rec, f"{name}.compact{tag}", T.COMPACT_KEYS, c)
            assert np.array_equal(np.nan_to_num(mean64, nan=1.0)[c[4].numpy()] <= 0.02 + 1e-7, np.ones(len(c[4]), bool))
            w = helper.batch_subdivide_volume(pos[None], tet[None], None if m is None else m[None])
            _put(rec, f"{name}.subdiv{tag}", T.SUBDIV_KEYS, w)
            d = helper.batch_subdivide_volume(c[0][None], c[2][None], None if m is None else c[3][None])
            _put(rec, f"{name}.chain{tag}", T.SUBDIV_KEYS, d)
        if name == "odd":                                    # the exact rows: 0.02f and -0.02f kept, the next float32 above dropped
            kept = set(c[4].tolist())
            assert {0, 1, 4, 5, 6} <= kept and not ({2, 3} & kept), sorted(kept)
        out = helper._forward(pos, sdf.clone(), tet)
        centroid = out["verts"][out["faces"]].mean(1)
        edit = (centroid[:, 0] > 0.5).int()
        assert 0 < int(edit.sum()) < len(edit)
        helper._grid_vertices, helper.indices = pos, tet
        mark = helper.mark_part_tets(None, sdf, edit)
        rec[f"{name}.edit_mask"] = edit.numpy()
        _put(rec, f"{name}.mark", T.MARK_KEYS, [mark[k] for k in T.MARK_KEYS])
        assert len(np.unique(s["pos"], axis=0)) == len(s["pos"])          # no two vertices share a position: membership by index is the reference's
        print(name, "N", len(pos), "F", len(tet), "closest gap to the threshold", float(gap[free].min()), "kept", len(c[4]), "vertices", len(c[0]), "edges of the kept",
              d[0].shape[1] - len(c[0]), "sub-tetrahedra", d[1].shape[1], "| whole scene: edges", w[0].shape[1] - len(pos), "| faces", len(edit), "edited", int(edit.sum()),
              "keep tets", len(mark["keep_tet_idx"]), "shared vertices", int(mark["mask_keep_part_in_new_pos"].sum()))
    np.savez_compressed(T.FIXTURE, **rec)
    print("wrote", T.FIXTURE, len(rec), "arrays,", os.path.getsize(T.FIXTURE) // 1024, "KiB")


if __name__ == "__main__":
    main()
