"""GPU: the mesh regions (youreditableavatar_amd.mesh_region, csrc/tgs_mesh_region.hip) against the restatement (tests/mesh_region_ref.py): every mask, label
and size bit for bit, on two runs and on a non-default stream, and the components loop ends below its cap on every mesh."""
import numpy as np
import pytest
import torch

from tests import mesh_region_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _icosphere(n):
    from youreditableavatar_amd import scenes
    v, f = scenes.icosphere(n)
    return v, f.astype(np.int32)


def _mesh(name):
    """-> (V, faces int32 [F,3], vertex positions or None)"""
    if name.startswith("icosphere"):
        v, f = _icosphere(int(name[-1]))
        return len(v), f, v
    if name == "two_icospheres":                                                # two disjoint icospheres
        v, f = _icosphere(2)
        return 2 * len(v), np.concatenate([f, f + len(v)]).astype(np.int32), None
    if name == "grid":                                                          # a 9 x 7 open grid
        return R.grid(9, 7) + (None,)
    if name == "bowtie":
        return R.bowtie() + (None,)
    if name == "fan":                                                           # three faces on one edge
        return R.fan_on_an_edge() + (None,)
    if name == "loose_ends":                                                    # unreferenced vertices, one duplicate face, a degenerate face, two faces with an index outside [0, V)
        V, f = R.grid(4, 3)
        f = np.concatenate([f, f[5:6], [[0, 0, 1]], [[0, 1, V + 7]], [[-1, 2, 3]], [[2, 3, 1 << 30]]]).astype(np.int32)
        return V + 5, f, None
    V, f = R.strip(int(name[1:]))                                               # F = 1, 63, 65, 257
    return V, f, None


MESHES = ["icosphere2", "icosphere3", "grid", "two_icospheres", "bowtie", "fan", "loose_ends", "F1", "F63", "F65", "F257"]


def _disc_hit(V, f, v):
    """the faces under a disc in a 64 x 64 raster, through the mesh rasterizer's hit_faces"""
    from youreditableavatar_amd import mesh_raster as dr
    pos = torch.from_numpy(np.concatenate([v[:, :2] * 0.8, v[:, 2:] * 0.5, np.ones((V, 1), np.float32)], axis=1).astype(np.float32)).to(DEV)
    tri = torch.from_numpy(f).to(DEV)
    rast, _ = dr.rasterize(None, pos[None], tri, (64, 64))
    yy, xx = np.mgrid[0:64, 0:64]
    disc = torch.from_numpy(((yy - 28) ** 2 + (xx - 36) ** 2) <= 9 ** 2).to(DEV)
    hit = dr.hit_faces(rast, disc, num_faces=len(f))
    assert hit.dtype == torch.bool and hit.shape == (len(f),) and 0 < int(hit.sum()) < len(f) // 2
    return hit.cpu().numpy()


def _selections(name, V, f, v):
    F = len(f)
    rng = np.random.default_rng(F)
    one = np.zeros(F, bool)
    one[F // 2] = True
    sels = {"empty": np.zeros(F, bool), "full": np.ones(F, bool), "one": one, "random": rng.random(F) < 0.1}
    if v is not None:
        sels["disc"] = _disc_hit(V, f, v)
    return sels


def _eq(got: torch.Tensor, want: np.ndarray) -> bool:
    return torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("name", MESHES)
def test_masks_labels_and_sizes_equal_the_restatement(name):
    from youreditableavatar_amd import mesh_region as mr
    V, f, v = _mesh(name)
    F = len(f)
    faces = torch.from_numpy(f).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    for sname, sel in _selections(name, V, f, v).items():
        s = torch.from_numpy(sel).to(DEV)
        torch.cuda.synchronize()

        n_sel = int(sel.sum())
        want = {("dilate", n): R.dilate_faces(sel, f, V, n) for n in (0, 1, 2, 5)}                         # the restatement, once per selection
        want.update({("erode", n): R.erode_faces(sel, f, V, n) for n in (0, 1, 2, 5)})
        want.update({("refine", d, e): R.refine_region(f, sel, V, d, e) for d, e in ((1, 2), (2, 5), (8, 10))})
        want["components"] = R.face_components(sel, f, V)
        want.update({("keep", m): (want["components"][0] >= 0) & (want["components"][1] >= m) for m in (1, 2, int(0.25 * n_sel))})

        def check(stream=None):
            what = (name, sname, "side stream" if stream else "current stream")
            for n in (0, 1, 2, 5):
                assert _eq(mr.dilate_faces(s, faces, V, n), want["dilate", n]), what + ("dilate", n)
                assert _eq(mr.erode_faces(s, faces, V, n), want["erode", n]), what + ("erode", n)
            for d, e in ((1, 2), (2, 5), (8, 10)):
                region = mr.refine_region(faces, s, V, d, e)
                assert region.face_mask.dtype == torch.bool and region.vertex_mask.shape == (V,)
                assert _eq(region.face_mask, want["refine", d, e][0]) and _eq(region.vertex_mask, want["refine", d, e][1]), what + ("refine", d, e)
            label, size = mr.face_components(s, faces, V)
            assert label.dtype == torch.int32 and size.dtype == torch.int32 and _eq(label, want["components"][0]) and _eq(size, want["components"][1]), what
            assert 0 < mr.last_component_rounds < F + 16                        # the loop ended below its cap
            for min_faces in (1, 2, int(0.25 * n_sel)):
                assert _eq(mr.keep_large_components(s, faces, V, min_faces), want["keep", min_faces]), what + (min_faces,)

        check()
        check()                                                                 # two runs
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):                                           # a non-default stream
            check(side)
        side.synchronize()


def test_hit_as_indices_the_default_iterations_and_the_empty_mesh():
    from youreditableavatar_amd import mesh_region as mr
    V, f, v = _mesh("icosphere2")
    faces = torch.from_numpy(f).to(DEV)
    hit = _disc_hit(V, f, v)
    idx = torch.from_numpy(np.nonzero(hit)[0]).to(DEV)
    by_mask, by_index = mr.refine_region(faces, torch.from_numpy(hit).to(DEV), V), mr.refine_region(faces, idx, V)
    want_f, want_v = R.refine_region(f, hit, V, 1, 2)                           # the defaults are the reference's (1, 2)
    assert _eq(by_mask.face_mask, want_f) and _eq(by_index.face_mask, want_f) and _eq(by_index.vertex_mask, want_v) and _eq(mr.refine_region(faces, idx.int(), V).vertex_mask, want_v)
    empty = mr.refine_region(faces, idx[:0], V, 8, 10)                          # an empty hit gives empty masks
    assert not bool(empty.face_mask.any()) and not bool(empty.vertex_mask.any())
    # the stage's use of the masks
    verts_mask = torch.ones(V, dtype=torch.bool, device=DEV)
    mask_dilate = (~by_mask.vertex_mask).float()[:, None]
    verts_mask &= ~by_mask.vertex_mask
    assert mask_dilate.shape == (V, 1) and int(verts_mask.sum()) == V - int(want_v.sum())
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)                     # no faces: empty masks, and no vertex is referenced
    region = mr.refine_region(none, torch.zeros(0, dtype=torch.bool, device=DEV), 5)
    assert region.face_mask.shape == (0,) and region.vertex_mask.shape == (5,) and not bool(region.vertex_mask.any())
    label, size = mr.face_components(torch.zeros(0, dtype=torch.bool, device=DEV), none, 5)
    assert label.shape == (0,) and size.shape == (0,)
    view = torch.from_numpy(np.concatenate([f, f], axis=1)).to(DEV)[:, 3:]      # a non-contiguous faces view
    assert _eq(mr.dilate_faces(torch.from_numpy(hit).to(DEV), view, V, 2), R.dilate_faces(hit, f, V, 2))
