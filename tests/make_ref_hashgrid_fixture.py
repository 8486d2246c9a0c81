#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Records what the reference's OWN code returns for the parts of the SDF field that it contains -- ``contract_to_unisphere``
(Edit_core/tetgs_spatial/models/geometry/base.py :14-26, ``unbounded=False``), ``VanillaMLP.forward`` (models/networks.py :151-188) and the mask schedule
of ``ProgressiveBandHashGrid.update_step`` (:97-106) -- into tests/golden/ref_hashgrid_fixture.npz.  The encoding itself has no reference code to
pin it (it is tiny-cuda-nn's, which is absent): between the reference's box map and the reference's network stands tests/hashgrid_ref.py's float64
restatement of the encoding, and the fixture says so by naming its arrays.

The two files are loaded from /root/reference by file path, with stub modules of a line each for the packages around them.  The fixture is data:
weights, inputs and outputs.  Every float input is a float32-representable number."""
import contextlib
import importlib.util
import os
import sys
import types
import typing

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import hashgrid_ref as R  # noqa: E402

OUT = R.FIXTURE
ROOT = "/root/reference/Edit_core/tetgs_spatial"
SCHEDULE = dict(start_level=2, start_step=100, update_steps=50)
STEPS = [0, 99, 100, 149, 150, 151, 349, 350, 10000]


class _Subscriptable:
    def __getitem__(self, item):
        return torch.Tensor


class _Encoding(torch.nn.Module):                       # tcnn.Encoding's place: the schedule reads n_output_dims alone
    def __init__(self, n_input_dims, config, dtype=None):
        super().__init__()
        self.n_output_dims = config["n_levels"] * config["n_features_per_level"]


def _module(name, **attrs):
    sys.modules[name] = mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    return mod


def _file(tag, path):
    spec = importlib.util.spec_from_file_location(tag, os.path.join(ROOT, path))
    sys.modules[tag] = mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load():
    names = _module("tetgs_spatial.utils.typing", Float=_Subscriptable(), Integer=_Subscriptable(), Int=_Subscriptable(), Bool=_Subscriptable(), Num=_Subscriptable(),
                    Tensor=torch.Tensor, DictConfig=dict)
    for k in ("Tuple", "Optional", "List", "Dict", "Any", "Union", "Callable"):
        setattr(names, k, getattr(typing, k))
    names.__all__ = [k for k in vars(names) if not k.startswith("_")]
    _module("tetgs_spatial", debug=lambda *a, **k: None, info=lambda *a, **k: None)
    _module("tetgs_spatial.utils")
    _module("igl", fast_winding_number_for_meshes=None, point_mesh_squared_distance=None, read_obj=None)
    _module("kaolin")
    _module("tinycudann", Encoding=_Encoding)
    base = _module("tetgs_spatial.utils.base", Updateable=type("Updateable", (), {}), BaseModule=type("BaseModule", (torch.nn.Module,), {"Config": type("Config", (), {})}))
    _module("tetgs_spatial.utils.config", config_to_primitive=lambda c: c)
    _module("tetgs_spatial.utils.misc", get_rank=lambda: "cpu")
    _module("tetgs_spatial.models")
    _module("tetgs_spatial.models.isosurface", IsosurfaceHelper=object, MarchingTetrahedraHelper=object)
    _module("tetgs_spatial.models.mesh", Mesh=object)
    sys.modules["tetgs_spatial.utils.ops"] = _file("tetgs_spatial.utils.ops", "utils/ops.py")
    return _file("ref_networks", "models/networks.py"), _file("ref_geometry_base", "models/geometry/base.py"), base


def main():
    networks, geometry, _ = _load()
    rec = {}
    for name in ("tiny", "odd"):
        levels = R.level_table(R.CONFIGS[name])
        H, D = R.MLP[name]
        C = 2 * len(levels)
        x, P = R.unbox(R.points(name, "uniform")[:257]), R.table(name)
        torch.manual_seed(R._seed(name, "fixture"))
        mlp = networks.VanillaMLP(C, D, {"n_neurons": H, "n_hidden_layers": 1})
        W1, W2 = mlp.layers[0].weight.detach().numpy().copy(), mlp.layers[2].weight.detach().numpy().copy()
        assert W1.dtype == np.float32 and W1.shape == (H, C) and W2.shape == (D, H) and mlp.layers[0].bias is None
        unit = geometry.contract_to_unisphere(torch.tensor(x), torch.tensor(R.BBOX, dtype=torch.float32), False)
        assert unit.dtype == torch.float32
        enc, _ = R.encode(unit.double(), torch.tensor(P).double(), levels)                     # the restatement, between the reference's two parts
        out = mlp.double()(enc) + R.FIXTURE_BIAS
        rec[f"{name}.x"], rec[f"{name}.params"], rec[f"{name}.W1"], rec[f"{name}.W2"] = x, P, W1, W2
        rec[f"{name}.unit_by_reference"], rec[f"{name}.enc_by_restatement"], rec[f"{name}.out_by_reference"] = unit.numpy(), enc.numpy(), out.detach().numpy()
        print(name, "points", len(x), "W1", W1.shape, "W2", W2.shape, "out range", float(out.min()), float(out.max()))
    cfg = dict(R.CONFIGS["default"], **SCHEDULE)
    torch.cuda.device = lambda *a: contextlib.nullcontext()      # (no device here: the constructor's device guard has nothing to guard)
    grid = networks.ProgressiveBandHashGrid(3, cfg)
    active = []
    for step in STEPS:
        grid.update_step(0, step)
        assert grid.mask[:grid.current_level * 2].all() and not grid.mask[grid.current_level * 2:].any()
        active.append(grid.current_level)
    rec["schedule.keys"], rec["schedule.steps"], rec["schedule.active_levels"] = np.array([SCHEDULE["start_level"], SCHEDULE["start_step"], SCHEDULE["update_steps"]]), np.array(STEPS), np.array(active)
    print("schedule", dict(zip(STEPS, active)))
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
