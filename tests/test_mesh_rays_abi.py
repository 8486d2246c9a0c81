"""CPU: the mesh ray casting at the C ABI and in youreditableavatar_amd.mesh_rays (no device needed): the header declares and the cross-compiled
library exports the entry points, the header states the rules, the signature table matches the headers, every refusal, the host twins in mode 0 against
mode 1 bit for bit and against the restatement under the bars, occlusion and the hit-face array against the cast, invalid rays, a corrupt tree, and
what the module refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_rays_ref as M
from tests import mesh_sdf_ref as R
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
TESTING = os.path.join(ROOT, "include", "tgs_mesh_rays_testing.h")         # included by tgs_raster_testing.h
PUBLIC = ("tgs_meshrays_cast", "tgs_meshrays_occluded")
HOST = ("tgs_meshrays_cast_host", "tgs_meshrays_occluded_host")
INVALID = -1
MAX_FACES = (1 << 28) - 1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import mesh_rays, mesh_sdf
    lib = mesh_sdf.declare(mesh_rays.declare(ctypes.CDLL(lib_path())))          # its own handle, the modules' signature tables
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def build_tree(lib, v, f):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    nbytes = lib.tgs_meshsdf_tree_bytes(len(f))
    tree = np.zeros(nbytes, np.uint8)
    assert lib.tgs_meshsdf_build(len(v), len(f), v.ctypes.data, f.ctypes.data, 0, tree.ctypes.data, nbytes) == 0, lib.tgs_last_error()
    return tree


def host_cast(lib, tree, v, f, rays, mode, hit_faces=None, faces_dtype=np.int32):
    """tgs_meshrays_cast_host -> (t_hit, face, geometry, uv, normal)"""
    v, f, rays = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, faces_dtype), np.ascontiguousarray(rays, np.float32)
    N = len(rays)
    out = (np.full(N, 7, np.float32), np.full(N, 7, np.int32), np.full(N, 7, np.int32), np.full((N, 2), 7, np.float32), np.full((N, 3), 7, np.float32))
    r = lib.tgs_meshrays_cast_host(tree.ctypes.data, tree.nbytes, len(v), len(f), v.ctypes.data, f.ctypes.data, int(faces_dtype == np.int64), N, rays.ctypes.data, mode,
                                   *(a.ctypes.data for a in out), hit_faces.ctypes.data if hit_faces is not None else None)
    assert r == 0, lib.tgs_last_error()
    return out


def host_occluded(lib, tree, v, f, rays, tnear, tfar, mode):
    v, f, rays = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(rays, np.float32)
    out = np.full(len(rays), 7, np.uint8)
    r = lib.tgs_meshrays_occluded_host(tree.ctypes.data, tree.nbytes, len(v), len(f), v.ctypes.data, f.ctypes.data, 0, len(rays), rays.ctypes.data, tnear, tfar, mode, out.ctypes.data)
    assert r == 0, lib.tgs_last_error()
    return out


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def is_miss(out, rows):
    t, face, geom, uv, normal = out
    return np.isposinf(t[rows]).all() and (face[rows] == -1).all() and (geom[rows] == -1).all() and not uv[rows].any() and not normal[rows].any()


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    testing = re.sub(r"/\*.*?\*/", "", open(TESTING).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(PUBLIC) <= declared and not set(HOST) & declared                  # the host twins are test-only
    assert all(name + "(" in testing for name in HOST)
    assert '#include "tgs_mesh_rays_testing.h"' in open(os.path.join(ROOT, "include", "tgs_raster_testing.h")).read()
    assert text.index("---- mesh regions ----") < text.index("---- mesh ray casting ----") < text.index("---- Batched backward")
    block = text[text.index("---- mesh ray casting ----"):text.index("---- Batched backward")]
    for rule in ("six float32", "not normalised", "units of |d|", "d == (0, 0, 0), is a miss", "nothing faults and nothing loops", "in double on the float32 inputs",
                 "largest |d_k| (the lowest axis on a tie)", "swapped when d[kz] < 0", "Sx = d[kx] / d[kz]", "Sz = 1 / d[kz]", "Ax = A[kx] - Sx * A[kz]", "Az = Sz * A[kz]",
                 "not of the face", "Woop", "U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax", "exact negatives", "cannot pass between them",
                 "exact zeros belong to both sides", "det = (U + V) + W", "det == 0 is no hit", "t = ((U * Az + V * Bz) + W * Cz) / det", "t >= 0 and t is finite",
                 "Both sides of a face are hit", "cross product (v1 - v0) x (v2 - v0), in double, is exactly zero is no hit", "zero-area\n * faces never hit",
                 "among equal t the lowest face index", "a total order", "rounded once", "(V / det, W / det)", "(1 - u - v) v0 + u v1 + v v2", "embree's", "normalised in double",
                 "t = +inf", "0xFFFFFFFF", "uvs and normals 0", "plain store", "accumulate the OR", "mode 1 visits every face in the caller's order", "skip links", "without a stack",
                 "layout order", "lo_k <= o_k <= hi_k", "(lo_k - o_k) / d_k and (hi_k - o_k) / d_k", "max(0, entries) <= min(best t so far, exits)", "ties are entered",
                 "bounded by the node count", "returns the bits of mode 1", "gives miss rows", "2^-20", "conservative", "|o_k| <= 64 m", "That is the range",
                 "tnear <= t <= tfar", "stops at the first such face", "no atomics, no LDS", "no scratch memory", "selects", "read nothing back", "two runs give the same bits",
                 "TGS_ERR_INVALID", "tnear > tfar or a NaN bound", "N == 0 returns without a launch", "tgs_mesh_rays_testing.h"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(PUBLIC + HOST) <= exported, sorted(set(PUBLIC + HOST) - exported)
    from youreditableavatar_amd import build, mesh_rays
    assert "tgs_mesh_rays.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["tgs_mesh_rays.hip"]
    assert set(mesh_rays.SIGNATURES) == set(PUBLIC + HOST)
    for name, (_, argtypes) in mesh_rays.SIGNATURES.items():                 # the table has as many arguments as the header's declaration, of the same kinds
        decl = re.search(name + r"\(([^;]*)\);", src + testing).group(1).split(",")
        assert len(argtypes) == len(decl), name
        for a, d in zip(argtypes, decl):
            want = ctypes.c_void_p if "*" in d else ctypes.c_float if "float" in d else ctypes.c_int64 if "int64_t" in d else ctypes.c_size_t if "size_t" in d else ctypes.c_int
            assert a is want, (name, d.strip())
    hpp = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_rays.hpp")).read()
    hip = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_rays.hip")).read()
    assert '#include "tgs_mesh_sdf.hpp"' in hpp and '#include "tgs_mesh_rays.hpp"' in hip and "struct Node" not in hpp and "build_tree" not in hip      # the tree is the SDF's
    for once in ("bool ray_face(", "bool ray_box(", "void cast_tree(", "void cast_brute(", "void occluded_tree(", "void occluded_brute("):              # one copy of each
        assert hpp.count(once) == 1 and once not in hip, once
    for banned in ("atomic", "stack[", "__shared__"):
        assert banned not in hpp.replace("without a stack", "") and banned not in hip.replace("without a stack", "").replace("no atomics", ""), banned
    assert not re.search(r"\b\w+\[(kx|ky|kz|k)\]", re.sub(r"//.*", "", hpp))    # no array indexed by an axis number: the permutation is selects
    assert os.path.exists(os.path.join(ROOT, "tools", "mesh_rays_host_check.cpp")) and "-fsanitize=address,undefined" in open(os.path.join(ROOT, "tools", "mesh_rays_host_check.cpp")).read()


def test_every_refusal():
    lib = _lib()
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    v, f = (np.ascontiguousarray(a) for a in R.SCENES["cube"]())
    tree = build_tree(lib, v, f)
    nbytes = tree.nbytes
    some = ctypes.c_void_p(4096)                                                # never dereferenced: the device calls must fail in the argument checks

    def cast(tree=some, nbytes=nbytes, V=8, F=12, vertices=some, faces=some, is64=0, N=4, rays=some, mode=0):
        return lib.tgs_meshrays_cast(None, tree, nbytes, V, F, vertices, faces, is64, N, rays, mode, some, some, some, some, some, some)

    def occluded(tree=some, nbytes=nbytes, V=8, F=12, vertices=some, faces=some, is64=0, N=4, rays=some, tnear=0.0, tfar=1.0, mode=0, out=some):
        return lib.tgs_meshrays_occluded(None, tree, nbytes, V, F, vertices, faces, is64, N, rays, tnear, tfar, mode, out)
    common = ((dict(tree=None), "non-NULL"), (dict(vertices=None), "non-NULL"), (dict(faces=None), "non-NULL"), (dict(rays=None), "non-NULL"), (dict(V=0), "V >= 1"), (dict(F=0), "1 <= F"),
              (dict(F=-3), "1 <= F"), (dict(F=MAX_FACES + 1), "1 <= F"), (dict(N=-1), "N >= 0"), (dict(is64=2), "faces_is_int64"), (dict(is64=-1), "faces_is_int64"),
              (dict(mode=2), "mode is 0"), (dict(mode=-1), "mode is 0"), (dict(nbytes=nbytes - 1), "smaller than"), (dict(nbytes=0), "smaller than"), (dict(N=1 << 40), "workgroups"))
    for kw, word in common:
        assert cast(**kw) == INVALID and "tgs_meshrays_cast:" in msg() and word in msg(), (kw, msg())
        assert occluded(**kw) == INVALID and "tgs_meshrays_occluded:" in msg() and word in msg(), (kw, msg())
    for kw, word in ((dict(tnear=1.0, tfar=0.5), "tnear <= tfar"), (dict(tnear=float("nan")), "NaN"), (dict(tfar=float("nan")), "NaN"), (dict(out=None), "out_occluded")):
        assert occluded(**kw) == INVALID and "tgs_meshrays_occluded:" in msg() and word in msg(), (kw, msg())
    assert cast(N=0) == 0 and cast(N=0, rays=None) == 0 and occluded(N=0) == 0 and occluded(N=0, rays=None, out=None) == 0        # N == 0: no launch, nothing is touched

    rays = np.ascontiguousarray(M.cube_tie_rays()[0])

    def hcast(tree=tree, nbytes=nbytes, V=8, F=12, is64=0, N=len(rays), rays=rays, mode=0):
        return lib.tgs_meshrays_cast_host(tree.ctypes.data if tree is not None else None, nbytes, V, F, v.ctypes.data, f.ctypes.data, is64, N, rays.ctypes.data if rays is not None else None, mode,
                                          None, None, None, None, None, None)

    def hocc(tree=tree, nbytes=nbytes, mode=0, tnear=0.0, tfar=1.0, out=np.zeros(len(rays), np.uint8)):
        return lib.tgs_meshrays_occluded_host(tree.ctypes.data if tree is not None else None, nbytes, 8, 12, v.ctypes.data, f.ctypes.data, 0, len(rays), rays.ctypes.data, tnear, tfar, mode,
                                              out.ctypes.data if out is not None else None)
    assert hcast() == 0 and hocc() == 0                                         # (every output of the cast may be NULL)
    for kw, word in ((dict(tree=None), "non-NULL"), (dict(rays=None), "non-NULL"), (dict(mode=2), "mode is 0"), (dict(nbytes=nbytes - 1), "smaller than"), (dict(V=0), "V >= 1"),
                     (dict(F=0), "1 <= F"), (dict(N=-1), "N >= 0"), (dict(is64=2), "faces_is_int64")):
        assert hcast(**kw) == INVALID and "tgs_meshrays_cast_host:" in msg() and word in msg(), (kw.keys(), msg())
    for kw, word in ((dict(tree=None), "non-NULL"), (dict(mode=2), "mode is 0"), (dict(nbytes=nbytes - 1), "smaller than"), (dict(tnear=2.0), "tnear <= tfar"),
                     (dict(tfar=float("nan")), "NaN"), (dict(out=None), "out_occluded")):
        assert hocc(**kw) == INVALID and "tgs_meshrays_occluded_host:" in msg() and word in msg(), (kw.keys(), msg())


@pytest.mark.parametrize("name", M.scene_names())
def test_host_twin_tree_equals_every_face_and_the_restatement(name):
    lib = _lib()
    v, f, rays, ref = M.scene(name)
    tree = build_tree(lib, v, f)
    hits = [np.zeros(len(f), np.uint8), np.zeros(len(f), np.uint8)]
    walk, brute = host_cast(lib, tree, v, f, rays, 0, hits[0]), host_cast(lib, tree, v, f, rays, 1, hits[1])
    assert same_bits(walk, brute) and np.array_equal(hits[0], hits[1])          # mode 0 equals mode 1 bit for bit
    t, face, geom, uv, normal = walk
    M.check_bars(v, f, rays, ref, t, face, uv, normal, what=name)
    assert np.array_equal(geom, np.where(face >= 0, 0, -1)) and is_miss(walk, slice(-3, None))               # the three invalid rays
    if name in ("cube", "body"):
        assert same_bits(host_cast(lib, tree, v, f, rays, 1, faces_dtype=np.int64), brute)                   # int64 indices are read as given
    # the hit faces are the set of returned faces, and a second call ORs into the first
    want = np.zeros(len(f), np.uint8)
    want[face[face >= 0]] = 1
    assert np.array_equal(hits[0], want)
    half = len(rays) // 2
    acc = np.zeros(len(f), np.uint8)
    host_cast(lib, tree, v, f, rays[:half], 0, acc)
    first = acc.copy()
    host_cast(lib, tree, v, f, rays[half:], 0, acc)
    early = np.zeros(len(f), np.uint8)
    early[face[:half][face[:half] >= 0]] = 1
    assert np.array_equal(first, early) and np.array_equal(acc, want) and (acc >= first).all()
    # occlusion is tnear <= t <= tfar of the cast, wherever there is no flag
    for tnear, tfar in ((0.0, np.inf), (0.5, 1.5), (1.0, 1.0), (-1.0, 0.75)):
        occ = [host_occluded(lib, tree, v, f, rays, tnear, tfar, mode) for mode in (0, 1)]
        assert np.array_equal(occ[0], occ[1]) and set(np.unique(occ[0])) <= {0, 1}
        inside = (ref["face"] >= 0) & (np.float32(tnear) <= ref["t"]) & (ref["t"] <= np.float32(tfar))
        if tnear <= 0.0:                                                        # the nearest hit is in [tnear, tfar] iff some hit is
            assert np.array_equal(occ[0][~ref["flag"]].astype(bool), inside[~ref["flag"]])
        assert occ[0][inside & ~ref["flag"]].all()                              # (with tnear > 0 a farther face inside the interval occludes too: the cube's test has that case in full)
    only_face = np.full(len(rays), 7, np.int32)                                 # each output may be NULL
    assert lib.tgs_meshrays_cast_host(tree.ctypes.data, tree.nbytes, len(v), len(f), v.ctypes.data, np.ascontiguousarray(f, np.int32).ctypes.data, 0, len(rays),
                                      np.ascontiguousarray(rays).ctypes.data, 0, None, only_face.ctypes.data, None, None, None, None) == 0
    assert np.array_equal(only_face, face)


def test_occlusion_against_every_face_of_the_cube():
    """the exact rule on a scene where it can be said in closed form: the faces a ray hits, by the restatement's pair function, and their t"""
    lib = _lib()
    v, f, rays, ref = M.scene("cube")
    tree = build_tree(lib, v, f)
    p = M.pairs(M.setup(rays)[1:], *(v[f[:, k]].astype(np.float64)[None] for k in range(3)))
    valid = M.setup(rays)[0]
    for tnear, tfar in ((0.0, np.inf), (0.5, 1.5), (1.0, 1.0), (2.0, 2.0), (-1.0, 0.75), (1.25, 3.0)):
        want = (p["hit"] & (p["t"] >= np.float32(tnear)) & (p["t"] <= np.float32(tfar))).any(axis=1) & valid
        for mode in (0, 1):
            assert np.array_equal(host_occluded(lib, tree, v, f, rays, tnear, tfar, mode).astype(bool), want), (tnear, tfar, mode)
    # tfar just below and just above a known hit: (0.25, 0.5, -2) along +z meets the cube at t = 2 and leaves it at t = 3
    ray = np.array([[0.25, 0.5, -2, 0, 0, 1]], np.float32)
    below, above = float(np.nextafter(np.float32(2), np.float32(0))), float(np.nextafter(np.float32(2), np.float32(4)))
    for mode in (0, 1):
        assert host_occluded(lib, tree, v, f, ray, 0.0, below, mode)[0] == 0 and host_occluded(lib, tree, v, f, ray, 0.0, 2.0, mode)[0] == 1
        assert host_occluded(lib, tree, v, f, ray, 0.0, above, mode)[0] == 1 and host_occluded(lib, tree, v, f, ray, above, 2.5, mode)[0] == 0
        assert host_occluded(lib, tree, v, f, ray, above, 3.0, mode)[0] == 1


def test_exact_ties_and_seams_on_the_host_twin():
    lib = _lib()
    v, f = R.SCENES["cube"]()
    rays, want_t = M.cube_tie_rays()
    ref = M.cast(v, f, rays)
    for mode in (0, 1):
        t, face, _, _, _ = host_cast(lib, build_tree(lib, v, f), v, f, rays, mode)
        assert np.array_equal(t, want_t.astype(np.float32)) and np.array_equal(face, ref["face"])
    v, f = R.SCENES["icosphere_1280"]()
    rays = M.icosphere_seam_rays(v, f)
    ref = M.cast(v, f, rays)
    tree = build_tree(lib, v, f)
    walk, brute = host_cast(lib, tree, v, f, rays, 0), host_cast(lib, tree, v, f, rays, 1)
    assert same_bits(walk, brute) and (walk[1] >= 0).all()                      # no ray leaks through a shared edge or a vertex
    assert np.array_equal(walk[1], ref["face"]) and np.array_equal(walk[0], ref["t_hit"])


def test_tree_shapes():
    lib = _lib()
    for name, nodes in (("triangle", 1), ("one_leaf", 1), ("one_leaf_and_one", 3)):
        v, f = R.SCENES[name]()
        assert int(build_tree(lib, v, f)[:64].view(np.uint32)[2]) == nodes, name


def test_a_corrupt_tree_gives_miss_rows_and_returns():
    lib = _lib()
    v, f, rays, ref = M.scene("icosphere_1280")
    good = build_tree(lib, v, f)
    assert not is_miss(host_cast(lib, good, v, f, rays, 0), slice(None))
    for word, value in ((0, 0), (1, len(f) + 1), (2, 2 * len(f) + 1)):          # the magic, the face count, a node count beyond the buffer
        tree = good.copy()
        tree[:64].view(np.uint32)[word] = value
        assert is_miss(host_cast(lib, tree, v, f, rays, 0), slice(None)), word
        assert not host_occluded(lib, tree, v, f, rays, 0.0, np.inf, 0).any()
        assert same_bits(host_cast(lib, tree, v, f, rays, 1), host_cast(lib, good, v, f, rays, 1))            # mode 1 does not read the tree
    # garbage behind a good header: skip links that point backwards, leaf words that do not fit, face numbers out of range.  Every call returns, no
    # output is written out of bounds (the hit-face array has a guard band), and the ids stay in [-1, F)
    rng = np.random.default_rng(5)
    F = len(f)
    for trial in range(4):
        tree = good.copy()
        body = tree[64:].view(np.int32)
        where = rng.integers(0, len(body), 4000)
        body[where] = rng.integers(-(1 << 31), 1 << 31, 4000, dtype=np.int64).astype(np.int32) if trial % 2 else rng.integers(-4, 4 * F, 4000).astype(np.int32)
        band = np.zeros(F + 128, np.uint8)
        v32, f32, r32 = np.ascontiguousarray(v), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(rays)
        face = np.full(len(rays), 7, np.int32)
        assert lib.tgs_meshrays_cast_host(tree.ctypes.data, tree.nbytes, len(v), F, v32.ctypes.data, f32.ctypes.data, 0, len(rays), r32.ctypes.data, 0, None, face.ctypes.data, None, None, None,
                                          band[64:].ctypes.data) == 0
        assert ((face >= -1) & (face < F)).all() and not band[:64].any() and not band[64 + F:].any()
        host_occluded(lib, tree, v, f, rays, 0.0, np.inf, 0)


def test_the_module_builds_on_the_host_and_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_rays as mr
    import youreditableavatar_amd.mesh_sdf as ms
    for word in ("no CPU path", "open3d", "no host read-back", "No autograd", "lowest face index", "inclusive", "zero-area faces never hit", "one mesh per scene", "double"):
        assert word in mr.__doc__, word
    assert mr.RaycastingScene.INVALID_ID == 4294967295 == np.uint32(np.int32(-1).view(np.uint32))
    v, f = R.icosphere(1)
    rays = np.zeros((2, 5, 6), np.float32)
    rays[..., 5] = 1
    for vertices, faces in ((v, f), (v.astype(np.float64), f.astype(np.int64)), (torch.from_numpy(v), torch.from_numpy(f)), (torch.from_numpy(v).double(), torch.from_numpy(f).long())):
        scene = mr.RaycastingScene()
        assert scene.add_triangles(vertices, faces) == 0 and scene.num_faces == len(f)
        with pytest.raises(RuntimeError, match="one mesh per scene"):
            scene.add_triangles(vertices, faces)                                # a second mesh
        short = mr.RaycastingScene(vertices, faces)
        assert np.array_equal(short._sdf._tree, scene._sdf._tree) and np.array_equal(short._sdf._tree, build_tree(_lib(), v, f))
        if not torch.cuda.is_available():                                       # no device: built, and a query is refused cleanly
            assert scene.device is None
            for call in (lambda: scene.cast_rays(rays), lambda: scene.test_occlusions(rays), lambda: scene.hit_faces(rays)):
                with pytest.raises(RuntimeError, match="on a HIP device only, and none is available"):
                    call()
        for call in (lambda: scene.cast_rays(torch.from_numpy(rays)), lambda: scene.hit_faces(torch.from_numpy(rays)), lambda: scene.test_occlusions(torch.from_numpy(rays))):
            with pytest.raises(RuntimeError, match="on a HIP device only, and none is available" if not torch.cuda.is_available() else "has no CPU path"):
                call()                                                          # a CPU tensor for rays
        with pytest.raises(RuntimeError, match=r"rays of shape \[...,6\]"):
            scene.cast_rays(np.zeros((3, 5), np.float32))
        with pytest.raises(RuntimeError, match=r"float32 rays of shape \[...,6\]"):
            scene.cast_rays(torch.zeros(3, 7))
        with pytest.raises(RuntimeError, match=r"float32 rays of shape \[...,6\]"):
            scene.cast_rays(torch.zeros(3, 6, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="mode is 0"):
            scene.cast_rays(rays, mode=2)
    scene = mr.RaycastingScene(v, f)
    for name in ("count_intersections", "list_intersections", "compute_closest_points", "compute_distance", "compute_signed_distance", "compute_occupancy"):
        with pytest.raises(NotImplementedError, match="does not serve " + name + ".*cast_rays.*mesh_sdf.SDF.closest"):
            getattr(scene, name)(rays)
    with pytest.raises(RuntimeError, match="no mesh"):
        mr.RaycastingScene().cast_rays(rays)
    with pytest.raises(RuntimeError, match="both or neither"):
        mr.RaycastingScene(v)
    with pytest.raises(RuntimeError, match="from_sdf takes"):
        mr.RaycastingScene.from_sdf(v)
    shared = mr.RaycastingScene.from_sdf(ms.SDF(v, f))
    assert shared.num_faces == len(f)
    with pytest.raises(RuntimeError, match="one mesh per scene"):
        shared.add_triangles(v, f)
    bad_f = f.copy()
    bad_f[3, 0] = len(v)
    with pytest.raises(RuntimeError, match=r"outside \[0, V\)"):
        mr.RaycastingScene(v, bad_f)


def test_a_cpu_tensor_for_rays_is_refused_by_name():
    """the message a CPU tensor gets where a device exists, from the same check: it comes after the shape checks and before any launch"""
    from youreditableavatar_amd import _host
    with pytest.raises(RuntimeError, match="youreditableavatar_amd.mesh_rays has no CPU path: rays must be on a HIP device"):
        _host.need_device("mesh_rays", rays=torch.zeros(2, 6))
    import inspect
    import youreditableavatar_amd.mesh_rays as mr
    assert '_need_device("mesh_rays", rays=rays)' in inspect.getsource(mr.RaycastingScene._rays)


def test_the_docs_have_the_ray_casting_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4s" in text and text.index("## 4r") < text.index("## 4s") < text.index("## 5. ")
    sec = text[text.index("## 4s"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.mesh_rays import RaycastingScene", "mesh_localization.py", "back_project", "generate_back_projection_rays", "o3d.core.Tensor",
                 "hit |= scene.hit_faces(rays)", "dr.hit_faces(rast", "just rasterized", "double", "lowest face index", "t >= 0", "zero-area", "one mesh per scene", "Nobody can run open3d",
                 "tools/mesh_rays_loop.py", "examples/back_project_rays.py", "tools/mesh_rays_host_check.cpp", "a record, not a bar", "layout order", "split axis",
                 "not built or measured", "from_sdf", "INVALID_ID"):
        assert what in sec, what
    fixed = text[text.index("## 4r"):text.index("## 4s")]
    assert "scene.hit_faces(rays)" in fixed                                     # 4r's row for mesh_localization.py :134 names the call that serves it
    for doc in ("README.md", "DESIGN.md", "SURVEY.md"):
        assert "mesh_rays" in open(os.path.join(ROOT, doc)).read(), doc
