"""CPU: the restatement of the mesh ray casting (tests/mesh_rays_ref.py) against closed forms -- the unit cube's exact hits and exact ties, the
icosphere's seams -- and the condition every shared scene must meet: at most 0.5 % of its rays carry the margin flag."""
import numpy as np
import pytest

from tests import mesh_rays_ref as M
from tests import mesh_sdf_ref as R


def rays_of(rows):
    return np.array(rows, np.float32)


@pytest.fixture(scope="module")
def cube():
    return R.SCENES["cube"]()


def test_axis_rays_from_dyadic_origins_hit_at_the_exact_t(cube):
    v, f = cube
    rows, want = [], []
    for k in range(3):
        for p in (0.125, 0.25, 0.625, 0.875):
            for q in (0.125, 0.5, 0.75):
                if p == q:
                    continue                                                    # (p == q is the diagonal: a tie, tested below)
                for start, step in ((-2.0, 1.0), (-0.75, 0.25), (3.5, -0.5)):
                    o, d = [0.0] * 3, [0.0] * 3
                    o[k], o[(k + 1) % 3], o[(k + 2) % 3], d[k] = start, p, q, step
                    rows.append(o + d)
                    want.append((0.0 - start) / step if step > 0 else (1.0 - start) / step)
    out = M.cast(v, f, rays_of(rows))
    assert np.array_equal(out["t"], np.array(want)) and (out["face"] >= 0).all() and not out["flag"].any()
    assert np.array_equal(out["t_hit"], np.array(want, np.float32))
    tri = v[f[out["face"]]].astype(np.float64)
    u, w = out["uv"][:, :1].astype(np.float64), out["uv"][:, 1:].astype(np.float64)
    r = rays_of(rows).astype(np.float64)
    assert np.array_equal((1 - u - w) * tri[:, 0] + u * tri[:, 1] + w * tri[:, 2], r[:, :3] + out["t"][:, None] * r[:, 3:])      # dyadic: the closure is exact
    n = out["normal"]
    assert np.array_equal(np.abs(n).sum(axis=1), np.ones(len(n))) and np.array_equal(np.abs(n[np.arange(len(n)), np.repeat(np.arange(3), len(n) // 3)]), np.ones(len(n)))


def test_exact_ties_hit_and_return_the_lowest_face(cube):
    v, f = cube
    rays, want_t = M.cube_tie_rays()
    out = M.cast(v, f, rays)
    assert np.array_equal(out["t"], want_t) and not out["flag"].any()
    p = M.pairs(M.setup(rays)[1:], *(v[f[:, k]].astype(np.float64)[None] for k in range(3)))
    tied = p["hit"] & (p["t"] == want_t[:, None])
    assert (tied.sum(axis=1) >= 2).all()                                        # every one of them is a tie between faces
    assert tied[4:].sum(axis=1).min() >= 3                                      # a corner: at least one face of each of its three sides
    assert np.array_equal(out["face"], np.argmax(tied, axis=1))                 # the lowest of the tied faces
    assert out["face"][0] == 0 and tied[0, :2].all()                            # faces 0 and 1 share the -z side's diagonal


def test_origin_on_a_face_away_parallel_and_scaled(cube):
    v, f = cube
    on = M.cast(v, f, rays_of([[0.25, 0.5, 0.0, 0, 0, 1], [0.25, 0.5, 1.0, 0, 0, 1], [0.0, 0.25, 0.5, -1, 0, 0]]))
    assert np.array_equal(on["t"], [0.0, 0.0, 0.0]) and (on["face"] >= 0).all()             # t >= 0 is inclusive
    away = M.cast(v, f, rays_of([[0.25, 0.5, 2.0, 0, 0, 1], [-1, 0.5, 0.5, -1, 0.25, 0], [0.5, 0.5, 0.5, 0, 0, 0]]))
    assert np.isposinf(away["t"]).all() and (away["face"] == -1).all() and not away["uv"].any() and not away["normal"].any()
    # inside the plane z = 0 of faces 0 and 1, parallel to them: det == 0, they are missed; the ray hits the side x = 0 at t = 1, on its edge
    flat = M.cast(v, f, rays_of([[-1.0, 0.5, 0.0, 1, 0, 0]]))
    p = M.pairs(M.setup(rays_of([[-1.0, 0.5, 0.0, 1, 0, 0]]))[1:], *(v[f[:, k]].astype(np.float64)[None] for k in range(3)))
    assert (p["det"][0, :2] == 0.0).all() and not p["hit"][0, :2].any()
    assert flat["t"][0] == 1.0 and flat["face"][0] >= 2
    base = rays_of([[-2.0, 0.3, 0.7, 1.0, 0.05, -0.1]])
    scaled = base.copy()
    scaled[:, 3:] *= 4
    a, b = M.cast(v, f, base), M.cast(v, f, scaled)
    assert a["face"][0] == b["face"][0] >= 0 and b["t"][0] == a["t"][0] / 4 and np.array_equal(a["normal"], b["normal"])


def test_zero_area_faces_and_invalid_rays_never_hit():
    v, f = R.SCENES["cube_and_flat_faces"]()
    rays = np.concatenate([M.scene("cube_and_flat_faces")[2], rays_of([[0.25, 0.0, -1, 0, 0, 1], [0.75, 0.0, -1, 0, 0, 1]])])      # the last two: through the collinear face's line
    out = M.cast(v, f, rays)
    assert (out["face"] < 12).all() and (out["face"][-2:] >= 0).all()           # faces 12, 13, 14 have no area
    bad = M.cast(v, f, M.INVALID_RAYS)
    assert np.isposinf(bad["t_hit"]).all() and (bad["face"] == -1).all() and not bad["flag"].any()


def test_no_ray_leaks_through_a_seam_of_the_icosphere():
    v, f = R.SCENES["icosphere_1280"]()
    rays = M.icosphere_seam_rays(v, f)
    assert len(rays) == 642 + 1920
    out = M.cast(v, f, rays)
    assert (out["face"] >= 0).all() and np.isfinite(out["t"]).all()
    assert (np.abs(out["t"] - 1.0) < 1e-2).all()                                # d is the vertex or the midpoint itself: the hit is at it, a chord's sag away at most
    # (many of these carry the margin flag -- a ray from the centre at a vertex makes that vertex's sheared coordinates a rounding residue -- and all hit
    # all the same: the two faces of an edge see exact negatives, whatever the residue is)
    assert out["flag"].any()


@pytest.mark.parametrize("name", M.scene_names())
def test_the_flag_count_is_within_the_cap(name):
    v, f, rays, ref = M.scene(name)
    hits = int((ref["face"] >= 0).sum())
    print(f"{name}: {len(rays)} rays, {hits} hits, {int(ref['flag'].sum())} margin flags")
    assert 380 <= len(rays) <= 420 and ref["flag"].sum() <= 0.005 * len(rays)
    assert hits > 0 and (ref["face"][-3:] == -1).all()
    if name == "body":
        assert 40 <= hits <= len(rays) - 40                                     # both hits and misses occur
    assert M.check_bars(v, f, rays, ref, ref["t_hit"], ref["face"], ref["uv"], ref["normal"], what=name) == int(ref["flag"].sum())      # the restatement meets its own bars
