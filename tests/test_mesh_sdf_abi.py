"""CPU: the mesh signed distance at the C ABI and in youreditableavatar_amd.mesh_sdf (no device needed): the header declares and the cross-compiled
library exports the entry points, the header states the rules, the signature table matches the headers, every refusal, the invariants of the tree
the host build writes, the host twin of the query in mode 0 against mode 1 bit for bit and against the restatement under the bars, and what the
module refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_sdf_ref as R
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
TESTING = os.path.join(ROOT, "include", "tgs_mesh_sdf_testing.h")          # included by tgs_raster_testing.h
PUBLIC = ("tgs_meshsdf_tree_bytes", "tgs_meshsdf_max_faces", "tgs_meshsdf_build", "tgs_meshsdf_query")
NEW = PUBLIC + ("tgs_meshsdf_query_host",)
INVALID = -1
MAX_FACES = (1 << 28) - 1
NODE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("skip", "<i4"), ("leaf", "<i4")])
RECORD = np.dtype([("v", "<f4", 9), ("idx", "<i4", 3), ("face", "<i4"), ("pad", "<i4", 3)])


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import mesh_sdf
    lib = mesh_sdf.declare(ctypes.CDLL(lib_path()))          # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def build_tree(lib, v, f):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    nbytes = lib.tgs_meshsdf_tree_bytes(len(f))
    tree = np.full(nbytes, 0xAB, np.uint8)
    assert lib.tgs_meshsdf_build(len(v), len(f), v.ctypes.data, f.ctypes.data, 0, tree.ctypes.data, nbytes) == 0, lib.tgs_last_error()
    return tree


def host_query(lib, tree, v, f, points, mode):
    """tgs_meshsdf_query_host -> (sdf, face, closest, inside)"""
    v, f, points = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(points, np.float32)
    N = len(points)
    sdf, face, closest, inside = np.full(N, 7, np.float32), np.full(N, 7, np.int32), np.full((N, 3), 7, np.float32), np.full(N, 7, np.uint8)
    r = lib.tgs_meshsdf_query_host(tree.ctypes.data, tree.nbytes, len(v), len(f), v.ctypes.data, f.ctypes.data, 0, N, points.ctypes.data, mode,
                                   sdf.ctypes.data, face.ctypes.data, closest.ctypes.data, inside.ctypes.data)
    assert r == 0, lib.tgs_last_error()
    return sdf, face, closest, inside


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def body():
    return R.load_fixture()


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    testing = re.sub(r"/\*.*?\*/", "", open(TESTING).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(PUBLIC) <= declared, sorted(set(PUBLIC) - declared)
    assert "tgs_meshsdf_query_host" not in declared and "tgs_meshsdf_query_host(" in testing          # the host twin is test-only
    assert '#include "tgs_mesh_sdf_testing.h"' in open(os.path.join(ROOT, "include", "tgs_raster_testing.h")).read()
    assert text.index("---- tetrahedral grids ----") < text.index("---- mesh signed distance ----") < text.index("---- Batched backward")
    assert src.index("tgs_tet_subdivide_emit(") < src.index("tgs_meshsdf_tree_bytes(")
    block = text[text.index("---- mesh signed distance ----"):]
    block = block[:block.index("tgs_meshsdf_query(void* stream")]
    for rule in ("exact point-to-triangle distance", "cross product is exactly zero takes part as its three segments", "lowest face index", "rounded once\n * to float32",
                 "squared distances", "at least two of the three ray parities", "cyclic order", "E = (V_a - U_a)(p_b - U_b) - (V_b - U_b)(p_a - U_a)", "canonical\n * direction",
                 "the vertex with the lower index", "same strict sign", "-(V_b - U_b)", "(V_a - U_a)", "top-left rule", "counted once", "sum to zero", "edge values as\n * weights",
                 "does not depend on the faces' orientation", "majority", "the overlap outside", "pysdf's sign", "d == 0: sdf = +0.0 and inside", "non-finite query point",
                 "nothing faults and nothing loops", "no device call", "depth-first order", "skip[i + 1]", "rounded outward", "at most 4 faces", "at\n * most 32 by construction",
                 "two builds give the same bytes", "without a stack", "strictly greater", "ties are visited", "only grows and is bounded by the node count",
                 "same bits and the same face as mode 1", "No atomics", "no scratch", "two runs give the same bits", "reads\n * nothing back", "no read-back", "2^28 - 1",
                 "without contraction", "TGS_ERR_INVALID", "a non-finite vertex", "a vertex index outside [0, V)", "N == 0 returns without a launch", "tgs_mesh_sdf_testing.h"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, mesh_sdf
    assert "tgs_mesh_sdf.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["tgs_mesh_sdf.hip"]
    assert set(mesh_sdf.SIGNATURES) == set(NEW)
    for name, (_, argtypes) in mesh_sdf.SIGNATURES.items():                  # the table has as many arguments as the header's declaration, of the same kinds
        decl = re.search(name + r"\(([^;]*)\);", src + testing).group(1).split(",")
        decl = [] if [d.strip() for d in decl] == ["void"] else decl
        assert len(argtypes) == len(decl), name
        for a, d in zip(argtypes, decl):
            want = ctypes.c_void_p if "*" in d else ctypes.c_float if "float" in d else ctypes.c_int64 if "int64_t" in d else ctypes.c_size_t if "size_t" in d else ctypes.c_int
            assert a is want, (name, d.strip())
    hpp = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_sdf.hpp")).read()
    hip = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_sdf.hip")).read()
    assert "fp contract(off)" in hpp and '#include "tgs_mesh_sdf.hpp"' in hip
    for once in ("D3 closest_on_triangle(", "int crossing(", "double box_lower_bound(", "void point_tree(", "void point_brute("):      # the pair functions and the walks: one copy
        assert hpp.count(once) == 1 and once not in hip, once
    for banned in ("atomic", "stack[", "__shared__"):
        assert banned not in hpp.replace("without a stack", "") and banned not in hip.replace("without a stack", "").replace("no atomics", ""), banned


def test_every_refusal():
    lib = _lib()
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    assert lib.tgs_meshsdf_max_faces() == MAX_FACES
    assert lib.tgs_meshsdf_tree_bytes(0) == 0 and lib.tgs_meshsdf_tree_bytes(-1) == 0 and lib.tgs_meshsdf_tree_bytes(MAX_FACES + 1) == 0
    assert lib.tgs_meshsdf_tree_bytes(1) == 64 + 128 and lib.tgs_meshsdf_tree_bytes(MAX_FACES) == 64 + 128 * MAX_FACES
    v, f = R.cube()
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    nbytes = lib.tgs_meshsdf_tree_bytes(len(f))
    tree = np.zeros(nbytes, np.uint8)

    def build(V=8, F=12, vertices=v, faces=f, is64=0, tree=tree, nbytes=nbytes):
        return lib.tgs_meshsdf_build(V, F, vertices.ctypes.data if vertices is not None else None, faces.ctypes.data if faces is not None else None, is64,
                                     tree.ctypes.data if tree is not None else None, nbytes)
    nan_v, inf_v = v.copy(), v.copy()
    nan_v[3, 1], inf_v[7, 2] = np.nan, -np.inf
    high, low = f.copy(), f.copy()
    high[5, 2], low[0, 0] = 8, -1
    for kw, word in ((dict(vertices=None), "non-NULL"), (dict(faces=None), "non-NULL"), (dict(tree=None), "non-NULL"), (dict(F=0), "F >= 1"), (dict(F=-1), "F >= 1"), (dict(V=0), "V >= 1"),
                     (dict(F=MAX_FACES + 1), "above the limit"), (dict(is64=2), "faces_is_int64"), (dict(faces=high), "outside [0, V)"), (dict(faces=low), "outside [0, V)"),
                     (dict(V=7), "outside [0, V)"), (dict(vertices=nan_v), "not finite"), (dict(vertices=inf_v), "not finite"), (dict(nbytes=nbytes - 1), "smaller than"), (dict(nbytes=0), "smaller than")):
        assert build(**kw) == INVALID and "tgs_meshsdf_build" in msg() and word in msg(), (kw.keys(), msg())
    assert build() == 0
    assert lib.tgs_meshsdf_build(8, 12, v.ctypes.data, f.astype(np.int64).ctypes.data, 1, tree.ctypes.data, nbytes) == 0            # int64 indices are read as given
    f64 = f.astype(np.int64)
    f64[2, 1] = 1 << 32                                                         # 0 when read as 32 bits
    assert lib.tgs_meshsdf_build(8, 12, v.ctypes.data, f64.ctypes.data, 1, tree.ctypes.data, nbytes) == INVALID and "outside [0, V)" in msg()
    assert build() == 0

    pts = np.zeros((4, 3), np.float32)
    some = ctypes.c_void_p(4096)                                                # never dereferenced: the device query must fail in the argument checks
    def query(tree=some, nbytes=nbytes, V=8, F=12, vertices=some, faces=some, is64=0, N=4, points=some, mode=0):
        return lib.tgs_meshsdf_query(None, tree, nbytes, V, F, vertices, faces, is64, N, points, mode, some, some, some, some)
    for kw, word in ((dict(tree=None), "non-NULL"), (dict(vertices=None), "non-NULL"), (dict(faces=None), "non-NULL"), (dict(points=None), "non-NULL"), (dict(F=0), "1 <= F"),
                     (dict(F=MAX_FACES + 1), "1 <= F"), (dict(V=0), "V >= 1"), (dict(N=-1), "N >= 0"), (dict(is64=-1), "faces_is_int64"), (dict(mode=2), "mode is 0"), (dict(mode=-1), "mode is 0"),
                     (dict(nbytes=nbytes - 1), "smaller than"), (dict(N=1 << 40), "workgroups")):
        assert query(**kw) == INVALID and "tgs_meshsdf_query" in msg() and word in msg(), (kw, msg())
    assert query(N=0) == 0 and query(N=0, points=None) == 0                     # N == 0: no launch, nothing is touched

    def hquery(tree=tree, nbytes=nbytes, mode=0, points=pts, N=4):
        out = np.zeros(4, np.float32)
        return lib.tgs_meshsdf_query_host(tree.ctypes.data if tree is not None else None, nbytes, 8, 12, v.ctypes.data, f.ctypes.data, 0, N, points.ctypes.data if points is not None else None,
                                          mode, out.ctypes.data, None, None, None)
    assert hquery() == 0
    for kw, word in ((dict(tree=None), "non-NULL"), (dict(points=None), "non-NULL"), (dict(mode=2), "mode is 0"), (dict(nbytes=nbytes - 1), "smaller than"),
                     (dict(tree=np.zeros(nbytes, np.uint8)), "was not built")):
        assert hquery(**kw) == INVALID and "tgs_meshsdf_query_host" in msg() and word in msg(), (kw.keys(), msg())


def tree_parts(tree, F):
    head = tree[:64].view(np.uint32)
    nodes = tree[64:64 + 64 * F].view(NODE)
    records = tree[64 + 64 * F:64 + 128 * F].view(RECORD)
    return head, nodes, records


@pytest.mark.parametrize("scene", ["triangle", "cube", "icosphere_1280", "body"])
def test_tree_invariants(scene, body):
    lib = _lib()
    v, f = dict(triangle=lambda: (R.cube()[0], R.cube()[1][:1]), cube=R.cube, icosphere_1280=lambda: R.icosphere(3), body=lambda: body[:2])[scene]()
    F = len(f)
    tree, again = build_tree(lib, v, f), build_tree(lib, v.copy(), f.copy())
    assert np.array_equal(tree, again)                                          # two builds give equal bytes (each over a buffer of 0xAB)
    head, nodes, records = tree_parts(tree, F)
    n_nodes, depth = int(head[2]), int(head[3])
    assert head[0] == 0x46445354 and head[1] == F and 1 <= n_nodes <= 2 * F and depth <= 32 and head[4] == 4 and not head[5:].any()
    assert not tree[64 + 32 * n_nodes:64 + 64 * F].any()                        # the unused nodes are zero
    nodes = nodes[:n_nodes]
    own = np.arange(n_nodes)
    assert (nodes["skip"] > own).all() and (nodes["skip"] <= n_nodes).all() and nodes["skip"][0] == n_nodes
    leaf = nodes["leaf"] >= 0
    first, count = nodes["leaf"][leaf] >> 3, nodes["leaf"][leaf] & 7
    assert (nodes["leaf"][~leaf] == -1).all() and (count >= 1).all() and (count <= 4).all() and (nodes["skip"][leaf] == own[leaf] + 1).all()
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(count)[:-1]])) and count.sum() == F        # leaf by leaf, every record in exactly one leaf
    assert np.array_equal(np.sort(records["face"]), np.arange(F))               # every face exactly once
    assert np.array_equal(records["idx"], f[records["face"]]) and np.array_equal(records["v"].reshape(F, 3, 3), v[f[records["face"]]])
    owner = np.repeat(own[leaf], count)                                         # the leaf of every record
    for lo, hi in zip(first, first + count):
        assert (np.diff(records["face"][lo:hi]) > 0).all()                      # ascending inside a leaf
    rv = records["v"].reshape(F, 3, 3)
    assert (rv > nodes["lo"][owner][:, None, :]).all() and (rv < nodes["hi"][owner][:, None, :]).all()      # strictly: the boxes are rounded outward
    # the left child is i + 1, the right child is skip[i + 1]; a parent's box holds its children's; the depth is what the header says, within the bound
    level, deepest = np.zeros(n_nodes, np.int64), 0
    for i in np.nonzero(~leaf)[0]:
        l = i + 1
        r = int(nodes["skip"][l])
        assert r < n_nodes and nodes["skip"][r] == nodes["skip"][i]
        for c in (l, r):
            level[c] = level[i] + 1
            assert (nodes["lo"][i] <= nodes["lo"][c]).all() and (nodes["hi"][i] >= nodes["hi"][c]).all()
    deepest = int(level.max())
    assert deepest == depth <= 32 and deepest <= int(np.ceil(np.log2(max(F, 1)))) + 1
    pad = 2.0 ** -20 * float(np.abs(v).max())
    assert ((rv.min(axis=1) - nodes["lo"][owner]) >= pad * 0.999).all() and ((rv.min(axis=1) - nodes["lo"][owner])[count[np.searchsorted(own[leaf], owner)] == 1] <= 1.01 * pad + 1e-6).all()


SCENES, scene_points = R.SCENES, R.scene_points


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_host_query_tree_equals_every_face_and_the_restatement(scene):
    lib = _lib()
    v, f = SCENES[scene]()
    pts = scene_points(v)
    tree = build_tree(lib, v, f)
    walk, brute = host_query(lib, tree, v, f, pts, 0), host_query(lib, tree, v, f, pts, 1)
    assert same_bits(walk, brute)
    R.check_bars(v, f, pts, R.query(v, f, pts), *walk, what=scene)
    only_face = np.full(len(pts), 7, np.int32)                                  # each output may be NULL; without sdf and inside the parities are not walked
    assert lib.tgs_meshsdf_query_host(tree.ctypes.data, tree.nbytes, len(v), len(f), v.ctypes.data, f.ctypes.data, 0, len(pts), pts.ctypes.data, 0, None, only_face.ctypes.data, None, None) == 0
    assert np.array_equal(only_face, walk[1])


def test_host_query_on_the_body_mesh(body):
    lib = _lib()
    v, f, pts, ref, flagged = body
    assert v.shape == (10475, 3) and f.shape == (20908, 3) and pts.shape == (4864, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert abs(float(np.abs(v).max()) - 0.9) < 1e-6 and flagged == int(ref["flag"].sum()) <= 0.005 * len(pts)
    assert os.path.getsize(R.FIXTURE) < 1000000
    tree = build_tree(lib, v, f)
    walk, brute = host_query(lib, tree, v, f, pts, 0), host_query(lib, tree, v, f, pts, 1)
    assert same_bits(walk, brute)                                               # mode 0 equals mode 1 bit for bit on every fixture point
    assert R.check_bars(v, f, pts, ref, *walk, what="body") == flagged
    assert (walk[0][-256:-170] == 0.0).all() and walk[3][-256:-170].all()       # the 86 points on vertices: d == 0, +0.0, inside
    split = ref["parity"].any(1) != ref["parity"].all(1)
    assert split.any() and np.array_equal(walk[3][split & ~ref["flag"]], ref["inside"][split & ~ref["flag"]])       # the mouth's hole: the majority settles them


def test_the_module_builds_on_the_host_and_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_sdf as ms
    assert "no CPU path" in ms.__doc__ and "pysdf" in ms.__doc__ and "no host read-back" in ms.__doc__ and "No autograd" in ms.__doc__
    v, f = R.icosphere(1)
    pts = np.zeros((3, 3), np.float32)
    for vertices, faces in ((v, f), (v.astype(np.float64), f.astype(np.int64)), (torch.from_numpy(v), torch.from_numpy(f)), (torch.from_numpy(v).double(), torch.from_numpy(f).long()),
                            (v, f.astype(np.uint32))):
        sdf = ms.SDF(vertices, faces)
        assert sdf.vertices.dtype == np.float32 and sdf.faces.dtype == np.int32 and np.array_equal(sdf.vertices, v) and np.array_equal(sdf.faces, f)
        assert np.array_equal(sdf._tree, build_tree(_lib(), v, f))
        if not torch.cuda.is_available():                                       # no device: built, and a query is refused cleanly
            assert sdf.device is None
            for call in (lambda: sdf(pts), lambda: sdf(torch.from_numpy(pts)), lambda: sdf.contains(pts), lambda: sdf.closest(pts)):
                with pytest.raises(RuntimeError, match="on a HIP device only, and none is available"):
                    call()
        with pytest.raises(RuntimeError, match=r"points of shape \[N,3\]"):
            sdf(np.zeros((3, 2), np.float32))
        with pytest.raises(RuntimeError, match=r"float32 points of shape \[N,3\]"):
            sdf(torch.zeros(3, 3, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="mode is 0"):
            sdf(pts, mode=2)
    sdf = ms.SDF(v, f)
    with pytest.raises(RuntimeError, match="robust=False"):
        ms.SDF(v, f, robust=False)
    for call, name in ((lambda: sdf.nn(pts), "nn"), (lambda: sdf.sample_surface(10), "sample_surface"), (lambda: sdf.surface_area, "surface_area")):
        with pytest.raises(RuntimeError, match="does not serve " + name):
            call()
    with pytest.raises(RuntimeError, match="faces has 0 rows"):
        ms.SDF(v, f[:0])
    bad_f, bad_v = f.copy(), v.copy()
    bad_f[3, 0], bad_v[5, 1] = len(v), np.nan
    with pytest.raises(RuntimeError, match=r"outside \[0, V\)"):
        ms.SDF(v, bad_f)
    with pytest.raises(RuntimeError, match="not finite"):
        ms.SDF(bad_v, f)
    with pytest.raises(RuntimeError, match=r"vertices of shape \[V,3\]"):
        ms.SDF(v[:, :2], f)
    with pytest.raises(RuntimeError, match=r"faces of shape \[F,3\] and an integer type"):
        ms.SDF(v, f.astype(np.float32))


def test_the_docs_have_the_mesh_sdf_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4q" in text and text.index("## 4p") < text.index("## 4q") < text.index("## 5. ")
    sec = text[text.index("## 4q"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.mesh_sdf import SDF", "initialize_shape", "points_rand", "pysdf", "nearest vertex", "Nobody could run pysdf", "majority", "overlap",
                 "robust=False", "nn", "sample_surface", "surface_area", "no host read-back", "tools/mesh_sdf_loop.py", "a record, not a bar", "Measured", "not measured",
                 "tools/mesh_sdf_host_check.cpp", "examples/init_sdf_from_mesh.py", "trimesh"):
        assert what in sec, what
    assert "mesh_sdf" in open(os.path.join(ROOT, "README.md")).read()
    survey = open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "mesh_sdf" in survey[survey.index("3.5"):]
