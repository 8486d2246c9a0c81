"""CPU: the restatement of the mesh regions (tests/mesh_region_ref.py) on hand meshes: the strict and the loose rule, the boundary, vertex-only contact,
a non-manifold edge, unreferenced vertices, faces with an index outside the mesh.  Then the launch cases: ``face_components_fast`` against the union-find,
and each case's keys, table load, busiest edge, components and reach counted in numpy."""
import numpy as np
import pytest

from tests import mesh_region_ref as R


def test_strip_erosion_of_a_full_selection_keeps_everything():
    V, f = R.strip(6)
    full = np.ones(len(f), bool)
    assert R.erode_faces(full, f, V, 1).all() and R.erode_faces(full, f, V, 5).all()          # boundary vertices whose incident faces are all selected stay marked
    assert R.dilate_faces(full, f, V, 3).all()
    one = np.zeros(len(f), bool)
    one[0] = True                                                               # face 0 = (0, 1, 2); vertex 2 is shared with faces 1 and 2
    assert list(np.nonzero(R.dilate_faces(one, f, V, 1))[0]) == [0, 1, 2]
    assert list(np.nonzero(R.dilate_faces(one, f, V, 2))[0]) == [0, 1, 2, 3, 4]
    assert not R.erode_faces(one, f, V, 1).any()                                # vertices 1 and 2 have an unselected face
    most = full.copy()
    most[5] = False                                                             # face 5 = (6, 5, 7): vertices 5 and 6 are lost, so faces 3 and 4 go
    assert list(np.nonzero(R.erode_faces(most, f, V, 1))[0]) == [0, 1, 2]
    assert np.array_equal(R.dilate_faces(one, f, V, 0), one) and np.array_equal(R.erode_faces(most, f, V, 0), most)


def test_bowtie_dilates_across_the_vertex_but_is_two_components():
    V, f = R.bowtie()
    one = np.array([True, False])
    assert R.dilate_faces(one, f, V, 1).all()
    label, size = R.face_components(np.ones(2, bool), f, V)
    assert list(label) == [0, 1] and list(size) == [1, 1]
    assert not R.keep_large_components(np.ones(2, bool), f, V, 2).any() and R.keep_large_components(np.ones(2, bool), f, V, 1).all()


def test_three_faces_on_one_edge_are_one_component():
    V, f = R.fan_on_an_edge()
    label, size = R.face_components(np.ones(3, bool), f, V)
    assert list(label) == [0, 0, 0] and list(size) == [3, 3, 3]
    label, size = R.face_components(np.array([False, True, True]), f, V)
    assert list(label) == [-1, 1, 1] and list(size) == [0, 2, 2]                # the label is the least index of the component, unselected faces get -1 and 0
    assert list(R.keep_large_components(np.array([False, True, True]), f, V, 2)) == [False, True, True]          # kept iff size >= min_faces
    assert not R.keep_large_components(np.array([False, True, True]), f, V, 3).any()


def test_unreferenced_vertices_duplicates_and_bad_indices():
    V, f = R.strip(4)
    f = np.concatenate([f, f[:1], [[0, 1, 99]], [[-1, 2, 3]]]).astype(np.int32)          # a duplicate of face 0 and two faces with an index outside [0, V)
    V += 3                                                                      # three vertices no face references
    face_mask, vertex_mask = R.refine_region(f, np.ones(len(f), bool), V, 0, 0)
    assert list(face_mask) == [True] * 5 + [False, False]                       # a face with a bad index is never selected
    assert vertex_mask[:6].all() and not vertex_mask[6:].any()                  # an unreferenced vertex is never in vertex_mask
    face_mask, vertex_mask = R.refine_region(f, np.ones(len(f), bool), V, 3, 3)
    assert list(face_mask) == [True] * 5 + [False, False] and not vertex_mask[6:].any()       # ... and touches no vertex: it does not block the erosion
    label, size = R.face_components(np.ones(len(f), bool), f, V)
    assert list(label) == [0, 0, 0, 0, 0, -1, -1] and list(size) == [5, 5, 5, 5, 5, 0, 0]     # the duplicate counts as a face
    empty, vempty = R.refine_region(f, np.zeros(len(f), bool), V, 8, 10)
    assert not empty.any() and not vempty.any()                                 # an empty hit gives empty masks
    by_index, _ = R.refine_region(f, np.array([0], np.int64), V, 1, 0)
    by_mask, _ = R.refine_region(f, np.arange(len(f)) == 0, V, 1, 0)
    assert np.array_equal(by_index, by_mask)


def test_degenerate_faces_and_the_grid():
    V, f = 4, np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3]], np.int32)             # (0, 0, 1): the side (0, 0) is no edge, (0, 1) is
    label, size = R.face_components(np.ones(3, bool), f, V)
    assert list(label) == [0, 0, 2] and list(size) == [2, 2, 1]
    V, f = R.grid(9, 7)
    assert V == 80 and len(f) == 126
    centre = np.zeros(len(f), bool)
    centre[2 * (3 * 9 + 4)] = True
    grown = R.dilate_faces(centre, f, V, 2)
    assert np.array_equal(R.refine_region(f, centre, V, 2, 2)[0], R.erode_faces(grown, f, V, 2)) and grown.sum() > 20
    assert R.erode_faces(grown, f, V, 1).sum() < grown.sum()
    two = centre.copy()
    two[0] = True
    label, size = R.face_components(two, f, V)
    assert sorted(set(label)) == [-1, 0, 2 * (3 * 9 + 4)] and size.max() == 1


# ---- the launch cases of tests/test_gpu_mesh_region_launch.py: the fast components and what each case is named for ----
def test_fast_components_equal_the_union_find_on_every_mesh_of_the_gpu_suite():
    pytest.importorskip("torch")
    from tests.test_gpu_mesh_region import MESHES, _mesh, _selections
    for name in MESHES:
        V, f, _ = _mesh(name)
        for sname, sel in _selections(name, V, f, None).items():                # (the disc selection needs the rasterizer: the GPU module checks it)
            slow, fast = R.face_components(sel, f, V), R.face_components_fast(sel, f, V)
            assert fast[0].dtype == np.int32 and fast[1].dtype == np.int32 and np.array_equal(slow[0], fast[0]) and np.array_equal(slow[1], fast[1]), (name, sname)
    V, f = R.grid(9, 7)
    for seed in range(5):                                                       # the 9 x 7 grid under random selections of every density
        sel = np.random.default_rng(seed).random(len(f)) < (0.2 + 0.15 * seed)
        assert all(np.array_equal(a, b) for a, b in zip(R.face_components(sel, f, V), R.face_components_fast(sel, f, V)))
    V, f = 4, np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [0, 1, 9]], np.int32)  # sides (i, i), a face with no edge at all, an index outside the mesh
    label, size = R.face_components_fast(np.ones(4, bool), f, V)
    assert list(label) == [0, 0, 2, -1] and list(size) == [2, 2, 1, 0]
    assert all(len(x) == 0 for x in R.face_components_fast(np.zeros(0, bool), np.zeros((0, 3), np.int32), 5))


def props(name, selection=None):
    V, f, sel = R.launch_case(name, selection)
    assert f.dtype == np.int32 and f.shape == (len(sel), 3) and sel.dtype == bool and f.min() >= 0 and f.max() < V
    p = R.case_properties(V, f, sel)
    assert p["capacity"] == R.table_capacity(len(f)) and p["capacity"] >= max(64, 4 * len(f)) and p["capacity"] & (p["capacity"] - 1) == 0
    assert p["capacity"] == 64 or p["capacity"] < 8 * len(f)                    # the power of two >= max(64, 4 F), restated
    return len(f), p


@pytest.mark.parametrize("n,order", [(4099, "reversed"), (4099, "random"), (4099, "evens_first"), (20000, "random")])
def test_permuted_strips(n, order):
    name = f"strip_{n}_{order}"
    F, p = props(name, "all")
    assert F == n and F % 256 == {4099: 3, 20000: 32}[n]                        # 16 workgroups and 3 lanes; 78 and 32 lanes
    assert p["keys"] == 2 * n + 1 and p["busiest"] == 2 and p["sizes"] == [n] and p["reach"] == n - 1
    assert sorted(map(tuple, R.launch_case(name, "all")[1])) == sorted(map(tuple, R.strip(n)[1]))          # the strip's faces, in another order
    F, p = props(name, "runs_of_96")
    cut = n // 97                                                               # the faces left out
    assert p["sizes"] == [96] * cut + [n - 97 * cut] and p["keys"] == 2 * (n - cut) + cut + 1 and p["busiest"] == 2
    assert p["reach"] == 95 if order == "reversed" else p["reach"] > n // 2     # (reversed keeps a run together: its least index is 95 rows away at most)


@pytest.mark.parametrize("n", [4096, 16384, 16385])
def test_isolated_triangles_fill_the_table_to_three_quarters(n):
    F, p = props(f"isolated_{n}", "all")
    assert F == n and p["keys"] == 3 * n and p["busiest"] == 1 and p["sizes"] == [1] * n and p["reach"] == 0
    if n & (n - 1) == 0:
        assert p["capacity"] == 4 * n and p["load"] == 0.75                     # the capacity rule's limit
    else:
        assert p["capacity"] == 8 * (n - 1) and 0.375 < p["load"] < 0.3751      # one face past the power of two: the capacity doubles
    F, p = props(f"isolated_{n}", "half")
    selected = int(R.launch_case(f"isolated_{n}", "half")[2].sum())
    assert 0.45 * n < selected < 0.55 * n and p["keys"] == 3 * selected and p["sizes"] == [1] * selected and p["busiest"] == 1


def test_pairs_book_and_spheres():
    F, p = props("pairs_16384")
    assert F == 16384 and p["keys"] == 5 * F // 2 and p["load"] == 0.625 and p["busiest"] == 2 and p["sizes"] == [2] * (F // 2) and p["reach"] > F // 2
    V, f, sel = R.launch_case("pairs_16384")
    label, _ = R.face_components_fast(sel, f, V)
    apart = np.nonzero(label != np.arange(F))[0]                                # the higher member of every pair
    assert len(apart) == F // 2 and (apart // 256 != label[apart] // 256).mean() > 0.95 and np.median(apart - label[apart]) > F // 8     # the members lie in different workgroups, far apart
    F, p = props("book_1000")
    assert F == 1000 and p["keys"] == 2 * F + 1 and p["busiest"] == 1000 and p["sizes"] == [1000] and p["reach"] == 999
    V, f, sel = R.launch_case("spheres_64", "random")
    whole = R.case_properties(V, f, np.ones(len(f), bool))
    assert len(f) == 64 * 320 and whole["sizes"] == [320] * 64 and whole["keys"] == 64 * 480 and whole["busiest"] == 2          # 64 closed spheres
    F, p = props("spheres_64", "random")
    assert 0.68 * F < sel.sum() < 0.72 * F and len(p["sizes"]) > 64 and len(set(p["sizes"])) >= 10 and p["sizes"][0] < 320 and p["sizes"][-1] == 1
    assert p["reach"] > F // 2                                                  # the rows of all copies are permuted together


def test_grids():
    F, p = props("grid_200x170", "all_but_middle")
    assert F == 68000 and -(-F // 256) == 266 and p["keys"] == 3 * 200 * 170 + 200 + 170 and p["sizes"] == [F - 1] and p["reach"] == F - 1
    F, p = props("grid_200x170", "middle")
    assert p["keys"] == 3 and p["sizes"] == [1]
    F, p = props("grid_200x170", "seeded")
    assert 40 < sum(p["sizes"]) < 100 and len(p["sizes"]) > 30
    V, f, sel = R.launch_case("grid_200x170", "seeded")
    assert R.case_properties(V, f, R.refine_region(f, sel, V, 8, 10)[0])["sizes"] == [16, 8, 4]          # what the localisation's chain leaves for the components
    V, f, sel = R.launch_case("grid_40x30_saturated", "middle")
    assert len(f) == 2400 and sel.sum() == 1 and not R.dilate_faces(sel, f, V, 20).all()
    full = R.dilate_faces(sel, f, V, 60)                                        # (the middle face lies at x = 0, row 15: the corner (40, 0) is 40 + 15 rings away)
    assert full.all() and R.erode_faces(full, f, V, 3).all()                    # saturated well before the 100 iterations; a full selection stays full under the strict rule
