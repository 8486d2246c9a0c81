"""The hash-grid field against what the reference's own functions returned (tests/golden/ref_hashgrid_fixture.npz, recorded by
tests/make_ref_hashgrid_fixture.py): ``contract_to_unisphere`` (the box map), ``VanillaMLP.forward`` (the network behind the encoding) and the mask
schedule of ``ProgressiveBandHashGrid``.  The encoding between the reference's two parts is tests/hashgrid_ref.py's restatement: tiny-cuda-nn, whose
encoding the reference calls, is nowhere to record from.  CPU: the restatement agrees with the recorded values; GPU: the fused field does, within the
project's bars (max error <= 4 eta with eta the float32 restatement's own error, rel-L2 <= 4x its)."""
import numpy as np
import pytest
import torch

from tests import hashgrid_ref as R
from tests.mesh_grad_ref import check_bars

NAMES = ("tiny", "odd")


def _restated(fx, name, dtype, cells=None):
    levels = R.level_table(R.CONFIGS[name])
    out, enc, _, cells = R.field(torch.tensor(fx[f"{name}.x"]), torch.tensor(fx[f"{name}.params"]).to(dtype), levels, torch.tensor(fx[f"{name}.W1"]).to(dtype),
                             torch.tensor(fx[f"{name}.W2"]).to(dtype), R.BBOX, R.FIXTURE_BIAS, None, cells)
    return out.double().numpy(), enc.double().numpy(), cells


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_agrees_with_the_reference_functions(name):
    fx = R.fixture()
    x = fx[f"{name}.x"]
    assert x.dtype == np.float32 and len(x) == 257 and fx[f"{name}.W1"].shape == (R.MLP[name][0], 2 * R.CONFIGS[name]["n_levels"]) and fx[f"{name}.W2"].shape == R.MLP[name][::-1]
    assert np.array_equal(R.box_map(torch.tensor(x), R.BBOX).numpy(), fx[f"{name}.unit_by_reference"])          # the fp32 box map, to the bit
    assert np.array_equal(fx[f"{name}.params"], R.table(name))
    out, enc, _ = _restated(fx, name, torch.float64)
    assert np.array_equal(enc, fx[f"{name}.enc_by_restatement"])
    np.testing.assert_allclose(out, fx[f"{name}.out_by_reference"], rtol=0, atol=1e-15)


def test_the_schedule_is_the_reference_classes():
    from youreditableavatar_amd import hashgrid
    fx = R.fixture()
    start_level, start_step, update_steps = (int(v) for v in fx["schedule.keys"])
    cfg = dict(R.CONFIGS["default"], otype="ProgressiveBandHashGrid", start_level=start_level, start_step=start_step, update_steps=update_steps)
    assert [hashgrid.progressive_levels(cfg, int(s)) for s in fx["schedule.steps"]] == fx["schedule.active_levels"].tolist()
    assert fx["schedule.active_levels"].tolist()[0] == start_level and fx["schedule.active_levels"].max() == 16


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_fused_field_against_the_reference_functions(name):
    from youreditableavatar_amd import hashgrid
    fx = R.fixture()
    dev = lambda k: torch.from_numpy(fx[f"{name}.{k}"].copy()).cuda()
    grid = hashgrid.HashGrid(3, R.CONFIGS[name]).cuda()
    with torch.no_grad():
        grid.params.copy_(dev("params"))
    mlp = torch.nn.Sequential(torch.nn.Linear(*fx[f"{name}.W1"].shape[::-1], bias=False), torch.nn.ReLU(inplace=True), torch.nn.Linear(*fx[f"{name}.W2"].shape[::-1], bias=False)).cuda()
    with torch.no_grad():
        mlp[0].weight.copy_(dev("W1")), mlp[2].weight.copy_(dev("W2"))
    field = hashgrid.SdfField(grid, mlp, bbox=R.BBOX, bias=R.FIXTURE_BIAS)
    assert field.fused
    with torch.no_grad():
        got = field(dev("x")).cpu().numpy()
    cells = _restated(fx, name, torch.float64)[2]                                 # (the float32 run takes the float64 run's cells, as everywhere)
    check_bars(f"{name} fused field against the reference's network", got, fx[f"{name}.out_by_reference"], _restated(fx, name, torch.float32, cells)[0])
