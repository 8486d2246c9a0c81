"""CPU: the restatement of the mesh regions (tests/mesh_region_ref.py) on hand meshes: the strict and the loose rule, the boundary, vertex-only contact,
a non-manifold edge, unreferenced vertices, faces with an index outside the mesh."""
import numpy as np

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
