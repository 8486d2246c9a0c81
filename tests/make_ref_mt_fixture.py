#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Records what the reference's OWN ``MarchingTetrahedraHelper._forward`` (Edit_core/tetgs_spatial/models/isosurface.py
:112-184) returns on the scenes of tests/mt_ref.py -- ``cases16``, ``fan``, ``kuhn_8`` -- in float64 on the CPU, into
tests/golden/ref_mt_fixture.npz: the three inputs and all five outputs per scene.

The class is loaded from /root/reference by file path, with stub modules for the package around it (its mesh class and its typing names are
all the file imports); the instance is built with ``object.__new__`` and carries the three tables its ``__init__`` registers, taken from a
throw-away subclass whose ``__init__`` is the original's up to the point where it reads a grid file.  The fixture is data: inputs and expected
outputs.  Every float input is a float32-representable number, so a float32 consumer starts from the same inputs.

Prints, per scene, the counts (valid tetrahedra, vertices, faces), the closed-manifold figures and the smallest |sdf| on a crossing edge."""
import importlib.util
import os
import sys
import types
import typing

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mt_ref as R  # noqa: E402

OUT = R.FIXTURE
SOURCE = "/root/reference/Edit_core/tetgs_spatial/models/isosurface.py"


class _Subscriptable:
    def __getitem__(self, item):
        return torch.Tensor


def _load_helper():
    names = types.ModuleType("tetgs_spatial.utils.typing")
    for k in ("Tuple", "Optional", "List", "Dict", "Any", "Union", "Callable"):
        setattr(names, k, getattr(typing, k))
    names.Float = names.Integer = names.Int = names.Bool = names.Num = _Subscriptable()
    names.Tensor = torch.Tensor
    mesh = types.ModuleType("tetgs_spatial.models.mesh")
    mesh.Mesh = object
    for name, mod in (("tetgs_spatial", types.ModuleType("tetgs_spatial")), ("tetgs_spatial.models", types.ModuleType("tetgs_spatial.models")),
                      ("tetgs_spatial.models.mesh", mesh), ("tetgs_spatial.utils", types.ModuleType("tetgs_spatial.utils")), ("tetgs_spatial.utils.typing", names)):
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("ref_isosurface", SOURCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MarchingTetrahedraHelper


def _instance(cls):
    """object.__new__ plus the three tables: the original __init__ registers them before it opens its grid file, which is not there"""
    obj = object.__new__(cls)
    torch.nn.Module.__init__(obj)
    try:
        cls.__init__(obj, 8, os.devnull)
    except Exception:                                        # noqa: BLE001 (np.load of no file: the tables are registered by then)
        pass
    for name, shape in (("triangle_table", (16, 6)), ("num_triangles_table", (16,)), ("base_tet_edges", (12,))):
        assert tuple(getattr(obj, name).shape) == shape, name
    return obj


def main():
    helper = _instance(_load_helper())
    rec = {}
    for name in R.FIXTURE_SCENES:
        s = R.scene(name)
        t64 = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=torch.float32).double()
        out = helper._forward(t64(s["pos"]), t64(s["sdf"]), torch.tensor(s["tet"]))
        rec[f"{name}.pos"], rec[f"{name}.sdf"], rec[f"{name}.tet"] = s["pos"], s["sdf"], s["tet"]
        for k in R.KEYS:
            rec[f"{name}.{k}"] = out[k].numpy()
        assert out["verts"].dtype == torch.float64 and out["faces"].dtype == torch.int64 and out["valid_tets"].dtype == torch.bool
        finite = np.isfinite(rec[f"{name}.verts"]).all(axis=1)
        print(name, "N", len(s["pos"]), "F", len(s["tet"]), "valid", int(out["valid_tets"].sum()), "verts", len(out["verts"]), "faces", len(out["faces"]),
              "NaN verts", int((~finite).sum()), "manifold", R.manifold_counts(out["faces"].numpy(), len(out["verts"])),
              "min |sdf| on a crossing edge", np.nanmin(np.abs(s["sdf"][out["interp_v"].numpy().reshape(-1)])))
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
