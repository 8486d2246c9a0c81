#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Records what the reference's OWN ``compute_normal`` (Edit_core/tetgs_spatial/models/renderers/nvdiff_rasterize_utils.py :12-35)
and ``Mesh`` (models/mesh.py: ``v_nrm``, ``edges``, ``normal_consistency()``, ``laplacian()``) return on the small scenes of tests/mesh_geom_ref.py --
``cases16``, ``fan``, ``kuhn_8``, ``traps`` -- in float64 on the CPU, into tests/golden/ref_mesh_geom_fixture.npz: the two inputs, the five outputs and the
``v_pos`` gradients of the three differentiable ones under the recorded upstreams.

The two files are loaded from /root/reference by file path, with stub modules for the package around them (a ``dot``, the typing names).  The
fixture is data: inputs and expected outputs.  Every float input is a float32-representable number, so a float32 consumer starts from the same
inputs.  No scene has exactly 3 faces (``torch.cross`` without ``dim`` would then cross along the wrong axis).

Prints, per scene, the counts and the scalar values."""
import importlib.util
import os
import sys
import types
import typing
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mesh_geom_ref as R  # noqa: E402

OUT = R.FIXTURE
ROOT = "/root/reference/Edit_core/tetgs_spatial/models"


class _Subscriptable:
    def __getitem__(self, item):
        return torch.Tensor


def _load():
    names = types.ModuleType("tetgs_spatial.utils.typing")
    for k in ("Tuple", "Optional", "List", "Dict", "Any", "Union", "Callable"):
        setattr(names, k, getattr(typing, k))
    names.Float = names.Integer = names.Int = names.Bool = names.Num = _Subscriptable()
    names.Tensor = torch.Tensor
    ops = types.ModuleType("tetgs_spatial.utils.ops")
    ops.dot = lambda x, y: torch.sum(x * y, -1, keepdim=True)
    top = types.ModuleType("tetgs_spatial")
    top.debug = top.info = lambda *a, **k: None
    for name, mod in (("tetgs_spatial", top), ("tetgs_spatial.utils", types.ModuleType("tetgs_spatial.utils")), ("tetgs_spatial.utils.typing", names),
                      ("tetgs_spatial.utils.ops", ops)):
        sys.modules[name] = mod
    mods = []
    for tag, path in (("ref_mesh", "mesh.py"), ("ref_nvdiff_utils", "renderers/nvdiff_rasterize_utils.py")):
        spec = importlib.util.spec_from_file_location(tag, os.path.join(ROOT, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[0].Mesh, mods[1].compute_normal


def main():
    Mesh, compute_normal = _load()
    warnings.simplefilter("ignore")                              # (torch.cross without dim is deprecated)
    rec = {}
    for name in R.FIXTURE_SCENES:
        m = R.scene(name)
        assert len(m["faces"]) != 3
        g = R.upstream(name, "random")
        rec[f"{name}.v_pos"], rec[f"{name}.faces"], rec[f"{name}.g_normals"], rec[f"{name}.g_scalar"] = m["v_pos"], m["faces"], g, np.asarray(R.SCALAR_UPSTREAM)
        leaf = lambda: torch.tensor(m["v_pos"]).double().requires_grad_(True)
        faces = torch.tensor(m["faces"])

        v = leaf()
        vn, _ = compute_normal(v, faces)
        (vn * torch.tensor(g).double()).sum().backward()
        rec[f"{name}.compute_normal"], rec[f"{name}.compute_normal.grad"] = vn.detach().numpy(), v.grad.numpy()

        v = leaf()
        mesh = Mesh(v, faces)
        rec[f"{name}.v_nrm"], rec[f"{name}.edges"] = mesh.v_nrm.detach().numpy(), mesh.edges.numpy()
        nc = mesh.normal_consistency()
        (nc * float(R.SCALAR_UPSTREAM)).backward()
        rec[f"{name}.normal_consistency"], rec[f"{name}.normal_consistency.grad"] = nc.detach().numpy(), v.grad.numpy()

        v = leaf()
        lap = Mesh(v, faces).laplacian()
        (lap * float(R.SCALAR_UPSTREAM)).backward()
        rec[f"{name}.laplacian"], rec[f"{name}.laplacian.grad"] = lap.detach().numpy(), v.grad.numpy()
        assert vn.dtype == torch.float64 and mesh.edges.dtype == torch.int64
        print(name, "V", len(m["v_pos"]), "F", len(m["faces"]), "E", len(mesh.edges), "self pairs", int((mesh.edges[:, 0] == mesh.edges[:, 1]).sum()),
              "normal_consistency", float(nc), "laplacian", float(lap), "non-finite gradient rows", int((~np.isfinite(rec[f'{name}.compute_normal.grad']).all(1)).sum()))
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
