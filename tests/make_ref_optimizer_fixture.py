#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Imports the reference's optimizer wrappers (Edit_core/tetgs_scene/tetgs_optimizer.py: OptimizationParams,
TetGSOptimizer, EditTetGSOptimizer) from /root/reference with stub modules in place of the packages this image lacks (none of them is
touched by the code exercised here), builds them over bare stand-in models carrying only the attributes the constructors read, and runs
the classes' OWN update_learning_rate() / step() on the CPU with seeded gradients, once with float32 and once with float64 parameters.
Recorded into tests/golden/ref_optimizer_fixture.npz, per model configuration:

    meta                      JSON: which wrapper, the OptimizationParams fields, spatial_lr_scale, the steps
    names, lr_iters, lrs      the group names in the optimizer's order; their learning rates after update_learning_rate(i) for several i
    init.<group>              the initial parameter (float32; the float64 run starts from the same values)
    grad.<group>, none.<group>   the gradient of every step (float32, used by both runs) and the steps on which .grad was None
    f32.* / f64.*             param, exp_avg, exp_avg_sq and step of every group after the last step

and ``sched.*``: position_sheduler_func at about 20 iterations.  A fixture is data: inputs and expected outputs."""
import json
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_optimizer_fixture.npz")
STEPS = 30
LR_ITERS = [0, 1, 2, 10, 29, 50, 100, 1000]
SCHED_ITERS = [-1, 0, 1, 2, 5, 10, 50, 100, 500, 1000, 2500, 7000, 15000, 29999, 30000, 30001, 60000, 1000000]


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return None


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def _stub_modules():
    for name in ("open3d", "pytorch3d", "pytorch3d.renderer", "pytorch3d.renderer.cameras", "pytorch3d.structures", "pytorch3d.transforms", "pytorch3d.ops",
                 "diff_gaussian_rasterization", "tetgs_scene.gs_model", "tetgs_scene.cameras", "PIL"):
        sys.modules[name] = _Stub(name)
    sys.path.insert(0, "/root/reference/Edit_core")


# configuration -> (wrapper, model flags the constructor reads, {group name: (model attribute, shape per Gaussian)}, P, OptimizationParams overrides, spatial_lr_scale)
def _configs():
    full = {"points": ("_points", (1,)), "sh_coordinates_dc": ("_sh_coordinates_dc", (1, 3)), "sh_coordinates_rest": ("_sh_coordinates_rest", (15, 3)),
            "all_densities": ("all_densities", (1,)), "scales": ("_scales", (3,)), "quaternions": ("_quaternions", (4,))}
    edit = {"points": ("_edit_points", (3,)), "sh_coordinates_dc": ("_edit_sh_coordinates_dc", (1, 3)), "all_densities": ("all_edit_densities", (1,)),
            "scales": ("_edit_scales", (3,)), "quaternions": ("_edit_quaternions", (4,))}
    return {
        # mesh-bound TetGS at four SH levels: all six groups
        "tetgs_L4": ("TetGSOptimizer", dict(binded_to_surface_mesh=True, learn_surface_mesh_positions=True, learn_positions=False, freeze_gaussians=False, sh_levels=4,
                                            learn_opacities=True, learn_surface_mesh_scales=True, learn_scales=False, learn_quaternions=False), full, 96,
                     dict(position_lr_max_steps=100), 3.7),
        # free Gaussians at one SH level with learn_opacities off: no "sh_coordinates_rest", no "all_densities"
        "tetgs_L1_no_opacity": ("TetGSOptimizer", dict(binded_to_surface_mesh=False, learn_surface_mesh_positions=False, learn_positions=True, freeze_gaussians=False, sh_levels=1,
                                                       learn_opacities=False, learn_surface_mesh_scales=False, learn_scales=True, learn_quaternions=True),
                                {k: (("_points", (3,)) if k == "points" else v) for k, v in full.items() if k not in ("sh_coordinates_rest", "all_densities")}, 192, dict(), 1.0),
        # the editing stage's wrapper at one SH level
        "edit_L1": ("EditTetGSOptimizer", dict(binded_to_surface_mesh=True, learn_positions=True, freeze_gaussians=False, edit_sh_levels=1, learn_opacities=True, learn_scales=True),
                    edit, 163, dict(iterations=2000, position_lr_max_steps=2000), 0.5),
    }


def _gradients(rng, groups, P):
    """[STEPS] gradients per group: a row is seen on 40 % of the steps (else exactly zero), rows 3, 10, 17, ... on none; magnitudes log-uniform
    in 1e-6 .. 1e2 per row and step.  The group after "sh_coordinates_dc" that exists has .grad = None on steps 2, 7, 12, ..."""
    out, none = {}, {}
    skipped = "all_densities" if "all_densities" in groups else "scales"
    for name, (_attr, shape) in groups.items():
        g = rng.standard_normal((STEPS, P) + shape) * 10.0 ** rng.uniform(-6, 2, (STEPS, P) + (1,) * len(shape))
        seen = rng.random((STEPS, P)) < 0.4
        seen[:, 3::7] = False
        out[name] = (g * seen.reshape((STEPS, P) + (1,) * len(shape))).astype(np.float32)
        none[name] = np.array([name == skipped and s % 5 == 2 for s in range(STEPS)])
    return out, none


def main():
    _stub_modules()
    from tetgs_scene import tetgs_optimizer as ref
    rng = np.random.Generator(np.random.PCG64(707))
    rec = {}
    for cname, (wrapper, flags, groups, P, over, scale) in _configs().items():
        init = {name: (rng.standard_normal((P,) + shape) * 0.5).astype(np.float32) for name, (_a, shape) in groups.items()}
        grads, none = _gradients(rng, groups, P)
        opt_params = ref.OptimizationParams(**over)
        rec[f"{cname}.meta"] = np.array(json.dumps(dict(wrapper=wrapper, opt={k: v for k, v in vars(opt_params).items()}, spatial_lr_scale=scale, steps=STEPS, P=P)))
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            model = types.SimpleNamespace(**flags)
            tensors = {}
            for name, (attr, _shape) in groups.items():
                tensors[name] = torch.nn.Parameter(torch.tensor(init[name], dtype=dt))
                setattr(model, attr, tensors[name])
            opt = getattr(ref, wrapper)(model, opt_params, spatial_lr_scale=scale)
            names = [g["name"] for g in opt.optimizer.param_groups]
            assert sorted(names) == sorted(groups), (names, sorted(groups))
            if tag == "f32":
                rec[f"{cname}.names"] = np.array(names)
                rows = []
                for it in LR_ITERS:
                    opt.update_learning_rate(it)
                    rows.append([float(g["lr"]) for g in opt.optimizer.param_groups])
                rec[f"{cname}.lr_iters"], rec[f"{cname}.lrs"] = np.array(LR_ITERS), np.array(rows, dtype=np.float64)
            for s in range(STEPS):
                opt.update_learning_rate()                    # (iteration = opt.current_iteration)
                for name, p in tensors.items():
                    p.grad = None if none[name][s] else torch.tensor(grads[name][s], dtype=dt)
                opt.step()
            assert opt.current_iteration == STEPS
            for name, p in tensors.items():
                st = opt.optimizer.state[p]
                rec[f"{cname}.{tag}.param.{name}"] = p.detach().numpy()
                rec[f"{cname}.{tag}.exp_avg.{name}"] = st["exp_avg"].numpy()
                rec[f"{cname}.{tag}.exp_avg_sq.{name}"] = st["exp_avg_sq"].numpy()
                rec[f"{cname}.{tag}.step.{name}"] = np.array(float(st["step"]))
        for name in groups:
            rec[f"{cname}.init.{name}"], rec[f"{cname}.grad.{name}"], rec[f"{cname}.none.{name}"] = init[name], grads[name], none[name]
    # the position schedule on its own: the defaults of the wrappers at spatial_lr_scale 3.7 (max_steps = 30 000, delay_mult given but no delay steps)
    d = ref.OptimizationParams()
    model = types.SimpleNamespace(binded_to_surface_mesh=False, learn_positions=False, freeze_gaussians=True, learn_opacities=True, learn_scales=False, learn_quaternions=False,
                                  learn_surface_mesh_positions=False, learn_surface_mesh_scales=False, all_densities=torch.nn.Parameter(torch.zeros(4, 1)))
    sched = ref.TetGSOptimizer(model, d, spatial_lr_scale=3.7).position_sheduler_func
    rec["sched.args"] = np.array(json.dumps(dict(lr_init=d.position_lr_init * 3.7, lr_final=d.position_lr_final * 3.7, lr_delay_mult=d.position_lr_delay_mult,
                                                 max_steps=d.position_lr_max_steps)))
    rec["sched.iters"], rec["sched.values"] = np.array(SCHED_ITERS), np.array([float(sched(i)) for i in SCHED_ITERS], dtype=np.float64)
    # and with a delay, straight from the function the wrappers call
    from utils.general_utils import get_expon_lr_func
    delayed = dict(lr_init=2e-3, lr_final=3e-5, lr_delay_steps=400, lr_delay_mult=0.05, max_steps=5000)
    f = get_expon_lr_func(**delayed)
    iters = [0, 1, 100, 399, 400, 401, 2500, 5000, 9000]
    rec["sched_delay.args"] = np.array(json.dumps(delayed))
    rec["sched_delay.iters"], rec["sched_delay.values"] = np.array(iters), np.array([float(f(i)) for i in iters], dtype=np.float64)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
