#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Records what the reference's OWN ``radii`` properties return -- ``TetGS.radii`` (Edit_core/tetgs_scene/tetgs_model.py:
299-310) and ``Edit3DTetGS.radii`` (tetgs_edit_3d.py:332-343), both through ``circumcircle_radius`` (utils/graphics_utils.py:109-116) -- on small
meshes with degenerate faces, and the value and autograd gradient of the scaling regulariser of the refinement loops
(tetgs_texture/refine.py:306-317, refine_3dgs.py:339-350) on the classes' own ``scaling`` / ``edit_scaling``, in float64 on the CPU, into
tests/golden/ref_scale_reg_fixture.npz.

The classes are imported from /root/reference with the stub modules of tests/make_ref_bind_fixture.py; ``pytorch3d.structures.Meshes`` gets a
stand-in that hands back the vertices and faces it was given, which is all the properties ask of it.  Instances are built with
``object.__new__`` and carry only what the properties read.  The loop's arithmetic is restated here (``loop_term``); the fixture is data:
inputs and expected outputs.

Every vertex and every raw scale is a float32-representable number (stored as float64), so a float32 consumer starts from the same inputs; the
scale sets are drawn so that no row lies within 1e-4 relative of either threshold (a consumer with float32 radii and a float32 ``exp`` decides
every row the same way), and hold two- and three-way ties of the maximum, which pin autograd's choice among equal maxima."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ref_bind_fixture import _bare, _stub_modules  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_scale_reg_fixture.npz")
SETTINGS = ((1.0, 10.0), (0.5, 0.5))                     # (max_factor, ratio_threshold): the loops' constants; one pair that lets isotropic rows through
MARGIN = 1e-4


class _Meshes:
    """the two accessors the radii properties call on a one-mesh batch"""

    def __init__(self, verts, faces, textures=None):
        self._verts, self._faces = verts[0], faces[0]

    def verts_packed(self):
        return self._verts

    def faces_packed(self):
        return self._faces


def loop_term(scaling, radii, max_factor, ratio_threshold):
    """refine.py:308-317 with its two constants as arguments -> (term or None when the loop adds nothing, the boolean row mask)"""
    big = scaling.max(dim=-1).values
    small = scaling.min(dim=-1).values
    mask = (big > radii * max_factor) & (big / small > ratio_threshold)
    return (big[mask].mean() if mask.sum() > 0 else None), mask


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_mesh(rng, V, F):
    verts = f32(rng.standard_normal((V, 3)) * 0.5)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int64)
    thin = np.arange(20, 40)                               # thin faces: the third vertex close to the first edge's line
    t = rng.uniform(0.2, 0.8, (len(thin), 1))
    verts[faces[thin, 2]] = f32(verts[faces[thin, 0]] * (1 - t) + verts[faces[thin, 1]] * t + rng.standard_normal((len(thin), 3)) * 3e-2)
    # degenerate faces.  Repeated vertices: 0 / 0 whatever the rounding.  Collinear: on an axis with dyadic steps, so that the side lengths
    # and s - c = 0 are exact.
    base = V - 6
    verts[base + 0] = [0.5, 1.0, 2.0]
    verts[base + 1] = [1.25, 1.0, 2.0]
    verts[base + 2] = [2.75, 1.0, 2.0]
    verts[base + 3] = [0.25, -0.5, 0.125]
    verts[base + 4] = [0.25, 1.0, 0.125]
    verts[base + 5] = [0.25, 4.0, 0.125]
    faces[0] = [faces[0, 0], faces[0, 0], faces[0, 2]]     # A == B
    faces[1] = [faces[1, 0], faces[1, 1], faces[1, 1]]     # B == C
    faces[2] = [faces[2, 0], faces[2, 1], faces[2, 0]]     # A == C
    faces[3] = [faces[3, 0]] * 3                           # one point
    faces[4] = [base + 0, base + 1, base + 2]              # collinear, C beyond B
    faces[5] = [base + 2, base + 0, base + 1]              # the same line, another order
    faces[6] = [base + 3, base + 5, base + 4]              # collinear, C between A and B
    return verts, faces


def make_raw_scales(rng, radii):
    """log-scales around the radii: flat rows (tetgs_edit_2d.py:203 stores log(1e-8) for the flat axis), isotropic rows, rows with a ratio around
    the threshold, two- and three-way ties; redrawn until every row keeps MARGIN from both thresholds of every setting"""
    P = radii.shape[0]
    r = np.where(np.isfinite(radii), np.minimum(radii, 5.0), 0.3)
    raw = np.empty((P, 3))

    def draw(i):
        kind = i % 6
        u = np.exp(rng.uniform(np.log(0.2), np.log(4.0), 3)) * r[i]
        if kind in (0, 1):
            s = np.array([1e-8, u[0], u[1]])
        elif kind == 2:
            s = u[0] * np.exp(rng.uniform(-0.5, 0.5, 3))
        elif kind == 3:
            s = u[0] * np.array([1.0, np.exp(rng.uniform(np.log(4.0), np.log(25.0))), 1.0]) / 4.0
        elif kind == 4:
            s = np.array([1e-8, u[0], u[0]])             # the initial state of a mesh-bound Gaussian: (1e-8, r, r)
        else:
            s = np.array([u[0], u[0], u[0]])
        s = s[rng.permutation(3)] if kind < 4 else s
        return f32(np.log(s))

    def safe(row, radius):
        s = np.exp(row)
        big, small = s.max(), s.min()
        for mf, rt in SETTINGS:
            if np.isfinite(radius) and abs(big / (radius * mf) - 1.0) < MARGIN:
                return False
            if abs(big / small / rt - 1.0) < MARGIN:
                return False
        return True

    for i in range(P):
        raw[i] = draw(i)
        while not safe(raw[i], radii[i]):
            raw[i] = draw(i)
        if i % 6 == 4:
            assert raw[i, 1] == raw[i, 2]
        if i % 6 == 5:
            assert raw[i, 0] == raw[i, 1] == raw[i, 2]
    return raw


def main():
    _stub_modules()
    sys.modules["pytorch3d.structures"].Meshes = _Meshes
    from tetgs_scene.tetgs_model import TetGS, scale_activation
    from tetgs_scene.tetgs_edit_3d import Edit3DTetGS
    rng = np.random.Generator(np.random.PCG64(808))
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    par = lambda a: torch.nn.Parameter(t64(a), requires_grad=True)
    rec = {}

    def record_terms(prefix, model, raw_name, scaling_of, radii):
        for k, (mf, rt) in enumerate(SETTINGS):
            scaling = scaling_of(model)
            scaling.retain_grad()
            term, mask = loop_term(scaling, radii, mf, rt)
            raw = getattr(model, raw_name)
            raw.grad = None
            if term is not None:
                term.backward()
            rec[f"{prefix}.set{k}.settings"] = np.array([mf, rt])
            rec[f"{prefix}.set{k}.value"] = np.array(0.0 if term is None else term.item())
            rec[f"{prefix}.set{k}.mask"] = mask.numpy()
            rec[f"{prefix}.set{k}.grad_scaling"] = np.zeros(tuple(scaling.shape)) if scaling.grad is None else scaling.grad.numpy().copy()
            rec[f"{prefix}.set{k}.grad_raw"] = np.zeros(tuple(raw.shape)) if raw.grad is None else raw.grad.numpy().copy()
        rec[f"{prefix}.scaling"] = scaling_of(model).detach().numpy()
        rec[f"{prefix}.raw_scales"] = getattr(model, raw_name).detach().numpy()

    # ---- TetGS: one Gaussian per face, and three per face (indices [P] and [P,1], int64 as the class keeps them) ----
    verts, faces = make_mesh(rng, 211, 300)
    for name, idx in (("tetgs.one", rng.permutation(300).astype(np.int64)), ("tetgs.three", np.repeat(np.arange(300, dtype=np.int64), 3)[:, None])):
        m = _bare(TetGS, _points_mesh=t64(verts), _surface_mesh_faces=torch.tensor(faces), _vertex_colors=torch.zeros(211, 3, dtype=torch.float64),
                  _face_indices=torch.tensor(idx), scale_activation=scale_activation)
        radii = m.radii.detach()                           # the class's own property
        assert radii.dtype == torch.float64 and radii.shape == (idx.shape[0],)
        m._scales = par(make_raw_scales(rng, radii.numpy()))
        rec[f"{name}.verts"], rec[f"{name}.faces"], rec[f"{name}.face_indices"], rec[f"{name}.radii"] = verts, faces, idx, radii.numpy()
        record_terms(name, m, "_scales", lambda mm: mm.scaling, radii)

    # ---- Edit3DTetGS: float-typed indices (tetgs_model.py:719), truncated by the property itself (tetgs_edit_3d.py:341); edit_scaling ----
    verts3, faces3 = make_mesh(rng, 157, 240)
    idx3 = np.repeat(rng.permutation(240), 3).astype(np.float32)
    e = _bare(Edit3DTetGS, _edit_surface_mesh=_Meshes([t64(verts3)], [torch.tensor(faces3)]), _edit_face_indices=torch.tensor(idx3, dtype=torch.float),
              bind_3dgs=True, scale_activation=scale_activation)
    radii3 = e.radii.detach()
    assert radii3.dtype == torch.float64 and radii3.shape == (720,)
    e._edit_scales = par(make_raw_scales(rng, radii3.numpy()))
    rec["edit3d.verts"], rec["edit3d.faces"], rec["edit3d.face_indices"], rec["edit3d.radii"] = verts3, faces3, idx3, radii3.numpy()
    record_terms("edit3d", e, "_edit_scales", lambda mm: mm.edit_scaling, radii3)

    for k in ("tetgs.one", "tetgs.three", "edit3d"):
        bad = ~np.isfinite(rec[f"{k}.radii"])
        print(k, "P", rec[f"{k}.radii"].shape[0], "non-finite radii", int(bad.sum()), "selected", [int(rec[f"{k}.set{s}.mask"].sum()) for s in range(len(SETTINGS))],
              "values", [float(rec[f"{k}.set{s}.value"]) for s in range(len(SETTINGS))])
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
