#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Writes tests/golden/ref_mesh_sdf_fixture.npz: the reference's body mesh as data and what the restatement
(tests/mesh_sdf_ref.py) answers for seeded query points.  The reference is read only here, and only for the mesh; the tests read the fixture.

The mesh: the ``v`` and ``f`` records of Edit_core/load/shapes/full_body.obj as float32 [V,3] and int32 [F,3], moved and scaled as
``ImplicitSDF.initialize_shape`` does it (Edit_core/tetgs_spatial/models/geometry/implicit_sdf.py :202-229 with the mesh as its own anchor, up
+z, front +x and shape_init_params 0.9: the centroid to the origin, +0.3 in y, the largest |coordinate| to 0.9), in float64, rounded once.

The points, 4 864 in all: 4 096 seeded ones, half uniform in [-1, 1]^3 and half uniform in the mesh's bounding box; 512 at seeded vertices moved
by +1e-3 or -1e-3 along the vertex normal; 256 exactly on the mesh: 86 vertices, 85 edge midpoints and 85 centroids, rounded to float32.

Asserts that at most 0.5 % of the points carry the restatement's margin flag, and writes the count into the fixture.  As written: 16 of 4 864
(0.33 %), all among the 256 points on the mesh, none among the 4 608 others.  The flag is set where a rounded sign decides ``inside``: a point at
distance exactly 0 (the 86 vertex points, 14 of the others) is inside by rule and carries none, and of the height rule only a COUNTED face -- one
above the point -- sets it.  With near misses below the point flagged too the count is 27 (0.56 %), and with the points at distance 0 on top 127."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mesh_sdf_ref as R  # noqa: E402

SOURCE = "/root/reference/Edit_core/load/shapes/full_body.obj"


def load_obj(path):
    v, f = [], []
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            v.append([float(x) for x in t[1:4]])
        elif t[0] == "f":
            idx = [int(x.split("/")[0]) - 1 for x in t[1:]]
            f += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    return np.array(v, np.float64), np.array(f, np.int32)


def main():
    v, faces = load_obj(SOURCE)
    v = v - v.mean(0)
    v[:, 1] += 0.3
    v = v / np.abs(v).max() * 0.9
    vertices = v.astype(np.float32)
    rng = np.random.default_rng(20261021)
    lo, hi = vertices.min(0), vertices.max(0)
    uniform = rng.uniform(-1.0, 1.0, (2048, 3))
    box = rng.uniform(lo, hi, (2048, 3))
    tri = vertices[faces].astype(np.float64)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, faces[:, k], fn)
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)
    pick = rng.choice(len(vertices), 512, replace=False)
    near = vertices[pick].astype(np.float64) + vn[pick] * np.where(np.arange(512) % 2 == 0, 1e-3, -1e-3)[:, None]
    on_v = vertices[rng.choice(len(vertices), 86, replace=False)]
    fe = faces[rng.choice(len(faces), 85, replace=False)]
    on_e = ((vertices[fe[:, 0]] + vertices[fe[:, 1]]) * np.float32(0.5)).astype(np.float32)
    fc = faces[rng.choice(len(faces), 85, replace=False)]
    on_c = ((vertices[fc[:, 0]].astype(np.float64) + vertices[fc[:, 1]] + vertices[fc[:, 2]]) / 3.0).astype(np.float32)
    points = np.concatenate([uniform, box, near, on_v, on_e, on_c]).astype(np.float32)
    kind = np.repeat(np.arange(6, dtype=np.int8), [2048, 2048, 512, 86, 85, 85])
    out = R.query(vertices, faces, points)
    flagged = int(out["flag"].sum())
    assert flagged <= 0.005 * len(points), (flagged, len(points))
    split = out["parity"].any(1) & ~out["parity"].all(1)
    rec = dict(vertices=vertices, faces=faces, points=points, kind=kind, flagged=np.int64(flagged), **{"out_" + k: a for k, a in out.items()})
    np.savez_compressed(R.FIXTURE, **rec)
    print("V", len(vertices), "F", len(faces), "points", len(points), "inside", int(out["inside"].sum()), "margin flags", flagged, "parities that disagree", int(split.sum()),
          "on the mesh (d < 1e-6)", int((out["dist"] < 1e-6).sum()), "| wrote", R.FIXTURE, os.path.getsize(R.FIXTURE) // 1024, "KiB")


if __name__ == "__main__":
    main()
