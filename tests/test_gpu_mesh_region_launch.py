"""GPU: the mesh regions (csrc/tgs_mesh_region.hip) at the launch shapes tests/test_gpu_mesh_region.py never reaches: ``R.LAUNCH_CASES``, each counted on
the CPU in tests/test_mesh_region_ref.py.  Every mask, label and size bit for bit against the restatement, on two runs and on a side stream.

  strip_*      a strip of 4 099 faces (16 workgroups and 3 lanes) and of 20 000 with its rows reversed, permuted, evens first: the hook and the jumps run
               across workgroups and the least index lies up to F - 1 rows from its neighbours; whole, and cut into runs of 96
  isolated_*   F triangles over 3 F vertices: 3 F keys in 4 F slots, the 3/4 load of the capacity rule, at F = 4 096 and 16 384, and one face past the
               power of two; every label is its own index, or a probe stopped at another key
  pairs_16384  8 192 pairs on one shared edge each, the members in different workgroups: 2.5 F keys in 4 F slots, a merge behind every shared key
  book_1000    1 000 faces on one edge: one slot with 1 000 pushers
  spheres_64   64 icospheres with all rows permuted together, 70 % selected: 744 components of 1 to 235 faces in one launch
  grid_200x170 68 000 faces, 266 workgroups that store the same epoch word to shared vertices: dilate to 40, erode, refine, and refine against
               erode(dilate) (the epoch counter runs on across the two phases); grid_40x30_saturated: 100 epochs on 2 400 faces

Rounds of the components loop.  Only the library's cap is asserted, 0 < rounds < F + 16: no tighter bound holds for an arbitrary schedule.  A synchronous
model of the rounds written from the kernels' text reaches the fixed point in 7 to 12 rounds on permuted strips of 4 099 to 65 536 faces and in 6 to 8 on
the 68 000-face grid.  The loop reads `changed` back once per 8 rounds, so what is printed is a multiple of 8.  Seen on the MI355X, the same on both runs
and on the side stream: 16 rounds on strip_4099_random and strip_20000_random with everything selected, 8 rounds on every other case and selection
(the other strips, whole and in runs of 96, isolated_*, pairs_16384, book_1000, spheres_64, the three patches of the grid's refine (8, 10)).  A change
after which a case here needs hundreds of rounds has made the loop slower by an order of magnitude."""
import numpy as np
import pytest
import torch

from tests import mesh_region_ref as R
from tests.test_gpu_mesh_region import DEV, _disc_hit, _eq, _mesh

pytestmark = pytest.mark.gpu
COMPONENT_CASES = [(name, selection) for name, (_, _, selections) in R.LAUNCH_CASES.items() if not name.startswith("grid") for selection in selections]
_grown = {}


def thrice(check):
    """two runs on the current stream and one on a side stream"""
    check("first run")
    check("second run")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        check("side stream")
    side.synchronize()


def check_components(tag, V, f, sel, keep=()):
    """face_components and keep_large_components at ``keep`` against the fast restatement -> the restatement's (label, size)"""
    from youreditableavatar_amd import mesh_region as mr
    F = len(f)
    faces, s = torch.from_numpy(f).to(DEV), torch.from_numpy(sel).to(DEV)
    want_label, want_size = R.face_components_fast(sel, f, V)
    torch.cuda.synchronize()

    def check(run):
        label, size = mr.face_components(s, faces, V)
        rounds = mr.last_component_rounds
        print(f"components {tag} F {F}, {run}: {rounds} rounds")
        assert label.dtype == torch.int32 and size.dtype == torch.int32 and _eq(label, want_label) and _eq(size, want_size), (tag, run)
        assert 0 < rounds < F + 16, (tag, run, rounds)                         # the loop ended below its cap
        for min_faces in keep:
            assert _eq(mr.keep_large_components(s, faces, V, min_faces), (want_label >= 0) & (want_size >= min_faces)), (tag, run, min_faces)

    thrice(check)
    return want_label, want_size


@pytest.mark.parametrize("name,selection", COMPONENT_CASES, ids=lambda x: str(x))
def test_components_equal_the_restatement(name, selection):
    V, f, sel = R.launch_case(name, selection)
    keep = ()
    if name == "spheres_64":
        _, size = R.face_components_fast(sel, f, V)
        sizes = R.case_properties(V, f, sel)["sizes"]
        keep = (1, int(np.median(sizes)), int(np.median(size[sel])), sizes[0] + 1)          # everything; the median over the components and over the faces; nothing
        assert keep[1] < keep[2] and 0.3 < (size >= keep[2]).sum() / sel.sum() < 0.7 and not (size >= keep[3]).any()
    label, size = check_components(f"{name} {selection}", V, f, sel, keep)
    rows = np.arange(len(f))
    if name.startswith("isolated"):                                             # what the GPU equalled: every label its own index, every size 1
        assert np.array_equal(label, np.where(sel, rows, -1)) and np.array_equal(size, sel.astype(np.int32))
    if name == "pairs_16384":                                                   # the lower member of the pair, size 2
        assert (size == 2).all() and (label <= rows).all() and (np.bincount(label) == 2).sum() == len(f) // 2
    if name == "book_1000":
        assert (label == 0).all() and (size == 1000).all()


def test_the_fast_restatement_on_the_disc_selections():
    """tests/test_mesh_region_ref.py compares ``face_components_fast`` with ``face_components`` on every selection of the sibling module but the disc, which
    the rasterizer makes"""
    for name in ("icosphere2", "icosphere3"):
        V, f, v = _mesh(name)
        hit = _disc_hit(V, f, v)
        assert all(np.array_equal(a, b) for a, b in zip(R.face_components(hit, f, V), R.face_components_fast(hit, f, V)))


def grown(selection, n):
    """R.dilate_faces(selection of the 200 x 170 grid, n) for n in 1, 2, 5, 8, 40: computed once, each from the one before"""
    if selection not in _grown:
        V, f, sel = R.launch_case("grid_200x170", selection)
        masks, at = {0: sel}, 0
        for upto in (1, 2, 5, 8, 40):
            masks[upto] = R.dilate_faces(masks[at], f, V, upto - at)
            at = upto
        _grown[selection] = masks
    return _grown[selection][n]


@pytest.mark.parametrize("selection", ["middle", "seeded"])
def test_grid_dilation_on_266_workgroups(selection):
    from youreditableavatar_amd import mesh_region as mr
    V, f, sel = R.launch_case("grid_200x170", selection)
    faces, s = torch.from_numpy(f).to(DEV), torch.from_numpy(sel).to(DEV)
    assert grown(selection, 40).sum() > grown(selection, 5).sum() > sel.sum()

    def check(run):
        for n in (1, 2, 5, 40):
            assert _eq(mr.dilate_faces(s, faces, V, n), grown(selection, n)), (selection, run, n)

    thrice(check)


def test_grid_erosion_of_the_complement():
    from youreditableavatar_amd import mesh_region as mr
    V, f, sel = R.launch_case("grid_200x170", "all_but_middle")
    faces, s = torch.from_numpy(f).to(DEV), torch.from_numpy(sel).to(DEV)
    want, at = {0: sel}, 0
    for n in (1, 2, 5):
        want[n] = R.erode_faces(want[at], f, V, n - at)
        at = n
    assert want[5].sum() < want[2].sum() < want[1].sum() < sel.sum()

    def check(run):
        for n in (1, 2, 5):
            assert _eq(mr.erode_faces(s, faces, V, n), want[n]), (run, n)

    thrice(check)


@pytest.mark.parametrize("selection", ["middle", "seeded"])
def test_grid_refine_equals_erode_of_dilate(selection):
    from youreditableavatar_amd import mesh_region as mr
    V, f, sel = R.launch_case("grid_200x170", selection)
    faces, s = torch.from_numpy(f).to(DEV), torch.from_numpy(sel).to(DEV)
    want = {(d, e): R.refine_region(f, sel, V, d, e) for d, e in ((1, 2), (2, 5), (8, 10))}
    if selection == "seeded":
        assert R.case_properties(V, f, want[8, 10][0])["sizes"] == [16, 8, 4]   # (from the middle face alone the ten erosions leave nothing)

    def check(run):
        for (d, e), (want_faces, want_vertices) in want.items():
            region = mr.refine_region(faces, s, V, d, e)
            assert region.face_mask.dtype == torch.bool and region.vertex_mask.shape == (V,)
            assert _eq(region.face_mask, want_faces) and _eq(region.vertex_mask, want_vertices), (selection, run, d, e)
            assert torch.equal(mr.erode_faces(mr.dilate_faces(s, faces, V, d), faces, V, e), region.face_mask), (selection, run, d, e)       # epochs d + 1 .. d + e against 1 .. e

    thrice(check)
    if selection == "seeded":                                                   # the localisation's chain: refine (8, 10), then the components of what is left
        check_components("grid_200x170 refine(8, 10) of seeded", V, f, want[8, 10][0], (1, int(0.25 * want[8, 10][0].sum())))


def test_saturated_grid_stays_full():
    from youreditableavatar_amd import mesh_region as mr
    V, f, sel = R.launch_case("grid_40x30_saturated", "middle")
    faces, s = torch.from_numpy(f).to(DEV), torch.from_numpy(sel).to(DEV)
    full = R.dilate_faces(sel, f, V, 100)
    assert full.all() and R.erode_faces(full, f, V, 100).all()

    def check(run):
        got = mr.dilate_faces(s, faces, V, 100)                                 # epochs far beyond the mesh's diameter
        assert _eq(got, full), run
        assert _eq(mr.erode_faces(got, faces, V, 100), full), run               # a full selection stays full under the strict rule
        region = mr.refine_region(faces, s, V, 100, 100)
        assert _eq(region.face_mask, full) and bool(region.vertex_mask.all()), run

    thrice(check)
