"""NumPy restatement of the rules of include/tgs_raster.h, "mesh regions": naive loops over the faces and the edges, components by a plain union-find.
The yardstick of youreditableavatar_amd.mesh_region; checked itself in tests/test_mesh_region_ref.py on hand meshes."""
import numpy as np


def valid_faces(faces, V):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < V)).all(axis=1)


def dilate_once(sel, faces, V):
    """VertexFromFaceLoose, then FaceFromVertexLoose"""
    ok = valid_faces(faces, V)
    marked = np.zeros(V, bool)
    for f in range(len(faces)):
        if sel[f] and ok[f]:
            for v in faces[f]:
                marked[v] = True
    out = np.zeros(len(faces), bool)
    for f in range(len(faces)):
        out[f] = ok[f] and any(marked[v] for v in faces[f])
    return out


def erode_once(sel, faces, V):
    """VertexFromFaceStrict, then FaceFromVertexStrict"""
    ok = valid_faces(faces, V)
    has_sel, has_unsel = np.zeros(V, bool), np.zeros(V, bool)
    for f in range(len(faces)):
        if ok[f]:
            for v in faces[f]:
                (has_sel if sel[f] else has_unsel)[v] = True
    marked = has_sel & ~has_unsel
    out = np.zeros(len(faces), bool)
    for f in range(len(faces)):
        out[f] = ok[f] and all(marked[v] for v in faces[f])
    return out


def _start(sel, faces, V):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.asarray(sel, bool).copy() & valid_faces(faces, V), faces


def dilate_faces(sel, faces, V, iterations=1):
    sel, faces = _start(sel, faces, V)
    for _ in range(iterations):
        sel = dilate_once(sel, faces, V)
    return sel


def erode_faces(sel, faces, V, iterations=1):
    sel, faces = _start(sel, faces, V)
    for _ in range(iterations):
        sel = erode_once(sel, faces, V)
    return sel


def refine_region(faces, hit, V, dilate_iter=1, erode_iter=2):
    """-> (face_mask [F], vertex_mask [V]); ``hit``: a bool [F] or an index array"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    hit = np.asarray(hit)
    if hit.dtype != bool:
        sel = np.zeros(len(faces), bool)
        sel[hit] = True
        hit = sel
    face_mask = erode_faces(dilate_faces(hit, faces, V, dilate_iter), faces, V, erode_iter)
    vertex_mask = np.zeros(V, bool)
    for f in np.nonzero(face_mask)[0]:
        vertex_mask[faces[f]] = True
    return face_mask, vertex_mask


def face_components(face_mask, faces, V):
    """-> (label int32 [F]: the least face index of the component, -1 if unselected; size int32 [F]).  Adjacent: a shared unordered pair of distinct indices."""
    sel, faces = _start(face_mask, faces, V)
    F = len(faces)
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}                                                                  # edge -> a face that has it
    for f in range(F):
        if not sel[f]:
            continue
        a, b, c = (int(x) for x in faces[f])
        for u, w in ((a, b), (b, c), (c, a)):
            if u == w:
                continue
            key = (min(u, w), max(u, w))
            if key in first:
                ra, rb = find(first[key]), find(f)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            else:
                first[key] = f
    label, size = np.full(F, -1, np.int32), np.zeros(F, np.int32)
    for f in range(F):
        if sel[f]:
            label[f] = find(f)                                                  # (the root is the least index: a union always hangs the larger root below the smaller)
    for f in range(F):
        if sel[f]:
            size[f] = int((label == label[f]).sum())
    return label, size


def keep_large_components(face_mask, faces, V, min_faces):
    label, size = face_components(face_mask, faces, V)
    return (label >= 0) & (size >= min_faces)


# ---- hand meshes ----
def strip(n=6):
    """a triangle strip of n faces over n + 2 vertices"""
    return n + 2, np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)], np.int32)


def bowtie():
    """two triangles that share vertex 2 only"""
    return 5, np.array([[0, 1, 2], [2, 3, 4]], np.int32)


def fan_on_an_edge():
    """three faces around the edge (0, 1): non-manifold"""
    return 5, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def grid(nx=9, ny=7):
    """an open grid of nx x ny quads, two triangles each"""
    idx = lambda x, y: y * (nx + 1) + x
    f = []
    for y in range(ny):
        for x in range(nx):
            f += [[idx(x, y), idx(x + 1, y), idx(x + 1, y + 1)], [idx(x, y), idx(x + 1, y + 1), idx(x, y + 1)]]
    return (nx + 1) * (ny + 1), np.array(f, np.int32)
