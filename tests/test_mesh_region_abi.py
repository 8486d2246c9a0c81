"""CPU: the mesh regions at the C ABI and in youreditableavatar_amd.mesh_region (no device needed): the header declares and the cross-compiled library
exports the entry points, the source is in build.SOURCES, the signature table matches the header, the header states the rules, and every refusal."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_meshregion_workspace_bytes", "tgs_meshregion_morph", "tgs_meshregion_components_workspace_bytes", "tgs_meshregion_components_max_rounds",
       "tgs_meshregion_components_begin", "tgs_meshregion_components_rounds", "tgs_meshregion_components_finish")
INVALID = -1
MAX_FACES = (1 << 28) - 1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import mesh_region
    lib = mesh_region.declare(ctypes.CDLL(lib_path()))          # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert text.index("---- mask morphology and blur ----") < text.index("---- mesh regions ----") < text.index("---- Batched backward")
    block = text[text.index("---- mesh regions ----"):text.index("---- Batched backward")]
    for rule in ("apply_selection_dilatation (VertexFromFaceLoose, then FaceFromVertexLoose), the loose rule", "a vertex is marked iff\n *              some incident face is selected",
                 "a face is selected iff any of its three vertices is marked", "apply_selection_erosion (VertexFromFaceStrict, then FaceFromVertexStrict), the strict rule",
                 "least one selected incident face and no unselected one", "a face stays selected iff all three of its vertices are marked",
                 "boundary vertex whose incident faces are all selected stays marked", "never selected and touches no vertex", "never read\n * through such an index",
                 "queued back to back with no read-back", "plain stores of a single value", "the same unordered pair of distinct vertex indices",
                 "non-manifold edge are all adjacent", "sharing only a vertex does not connect", "smallest face index", "gets -1 and 0", "size >= min_faces", "strictly smaller",
                 "Duplicate faces count as faces", "tgs_edge_set.hpp", "atomicMin", "label[f] = label[label[f]]", "reads `changed` back once per call of _rounds (8 rounds per call",
                 "nothing else is read back", "F rounds and one\n * quiet round always suffice", "stays below F + 16", "LAST round", "the loop never spins", "Integer atomics and plain stores only, no float anywhere",
                 "two runs give the same bits", "TGS_ERR_INVALID", "A degenerate face is an\n * ordinary face"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, mesh_region
    assert "tgs_mesh_region.hip" in build.SOURCES
    assert set(mesh_region.SIGNATURES) == set(NEW) and mesh_region.ROUNDS_PER_READBACK == 8
    for name, (_, argtypes) in mesh_region.SIGNATURES.items():                  # the table has as many arguments as the header's declaration, of the same kinds
        decl = re.search(name + r"\(([^;]*)\);", src).group(1).split(",")
        assert len(argtypes) == len(decl), name
        for a, d in zip(argtypes, decl):
            want = ctypes.c_void_p if "*" in d else ctypes.c_int64 if "int64_t" in d else ctypes.c_size_t if "size_t" in d else ctypes.c_int
            assert a is want, (name, d.strip())
    hip = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_region.hip")).read()
    assert "#define TGS_EDGE_SET_TABLE_ONLY" in hip and '#include "tgs_edge_set.hpp"' in hip and "edge_insert(" in hip
    assert "float" not in hip.replace("no float", "") and "double" not in hip   # integer decisions only


def test_every_refusal_of_the_library():
    lib = _lib()
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    assert lib.tgs_meshregion_workspace_bytes(100, 7) == 800 + 512 and lib.tgs_meshregion_workspace_bytes(-1, 7) == 0 and lib.tgs_meshregion_workspace_bytes(3, MAX_FACES + 1) == 0
    cw = lib.tgs_meshregion_components_workspace_bytes
    assert cw(-1) == 0 and cw(MAX_FACES + 1) == 0 and cw(0) >= 64 * 12 and cw(1000) >= 4096 * 12 + 1000 * 16          # 4 F = 4000 -> 4096 slots of a key and a label
    assert lib.tgs_meshregion_components_max_rounds(0) == 16 and lib.tgs_meshregion_components_max_rounds(1280) == 1296 and lib.tgs_meshregion_components_max_rounds(-1) == 0
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)                  # never dereferenced: every call must fail in the argument checks

    def morph(V=10, F=7, faces=some, sel_in=some, d=1, e=2, sel_out=other, vmask=None, ws=some, nbytes=1 << 20):
        return lib.tgs_meshregion_morph(None, V, F, faces, sel_in, d, e, sel_out, vmask, ws, nbytes)
    for kw, word in ((dict(V=-1), "V >= 0"), (dict(F=-1), "0 <= F"), (dict(F=MAX_FACES + 1), "0 <= F"), (dict(faces=None), "faces must be non-NULL"), (dict(sel_in=None), "sel_in and sel_out"),
                     (dict(sel_out=None), "sel_in and sel_out"), (dict(sel_out=some), "must not be sel_in"), (dict(d=-1), "dilate_iter, erode_iter"), (dict(e=-1), "dilate_iter, erode_iter"),
                     (dict(d=(1 << 20) + 1), "dilate_iter, erode_iter"), (dict(ws=None), "smaller than"), (dict(nbytes=80 + 511), "smaller than")):
        assert morph(**kw) == INVALID and "tgs_meshregion_morph" in msg() and word in msg(), (kw, msg())

    need = cw(7)
    def begin(V=10, F=7, faces=some, sel=some, label=some, ws=some, nbytes=need):
        return lib.tgs_meshregion_components_begin(None, V, F, faces, sel, label, ws, nbytes)
    for kw, word in ((dict(V=-1), "V >= 0"), (dict(F=MAX_FACES + 1), "0 <= F"), (dict(faces=None), "faces must be non-NULL"), (dict(sel=None), "sel and label"), (dict(label=None), "sel and label"),
                     (dict(ws=None), "smaller than"), (dict(nbytes=need - 1), "smaller than")):
        assert begin(**kw) == INVALID and "tgs_meshregion_components_begin" in msg() and word in msg(), (kw, msg())

    def rounds(F=7, label=some, done=0, n=8, changed=some, ws=some, nbytes=need):
        return lib.tgs_meshregion_components_rounds(None, F, label, done, n, changed, ws, nbytes)
    for kw, word in ((dict(F=-1), "0 <= F"), (dict(n=0), "1 <= rounds <= 16"), (dict(n=17), "1 <= rounds <= 16"), (dict(done=-1), "rounds_done >= 0"), (dict(done=23), "the cap of F + 16 rounds is reached"), (dict(done=40), "the loop ends here"),
                     (dict(label=None), "label and changed"), (dict(changed=None), "label and changed"), (dict(ws=None), "smaller than"), (dict(nbytes=need - 1), "smaller than")):
        assert rounds(**kw) == INVALID and "tgs_meshregion_components_rounds" in msg() and word in msg(), (kw, msg())

    def finish(F=7, label=some, size=some, ws=some, nbytes=need):
        return lib.tgs_meshregion_components_finish(None, F, label, size, ws, nbytes)
    for kw, word in ((dict(F=-1), "0 <= F"), (dict(label=None), "label and size"), (dict(size=None), "label and size"), (dict(ws=None), "smaller than"), (dict(nbytes=need - 1), "smaller than")):
        assert finish(**kw) == INVALID and "tgs_meshregion_components_finish" in msg() and word in msg(), (kw, msg())


def test_every_refusal_of_the_module():
    from youreditableavatar_amd import mesh_region as mr
    for word in ("no CPU path", "by coordinates", "by index", "duplicates count as faces", "two runs give the same bits", "reads one\nword back"):
        assert word in mr.__doc__, word
    faces, sel = torch.zeros(7, 3, dtype=torch.int32), torch.zeros(7, dtype=torch.bool)
    calls = {"dilate_faces": lambda f=faces, s=sel, V=10, **kw: mr.dilate_faces(s, f, V, **kw), "erode_faces": lambda f=faces, s=sel, V=10, **kw: mr.erode_faces(s, f, V, **kw),
             "refine_region": lambda f=faces, s=sel, V=10, **kw: mr.refine_region(f, s, V, **kw), "face_components": lambda f=faces, s=sel, V=10: mr.face_components(s, f, V),
             "keep_large_components": lambda f=faces, s=sel, V=10: mr.keep_large_components(s, f, V, 2)}
    for name, call in calls.items():
        for bad in (faces.long(), faces.float(), torch.zeros(7, 4, dtype=torch.int32), torch.zeros(21, dtype=torch.int32), faces.numpy()):
            with pytest.raises(RuntimeError, match=r"expected faces as an int32 tensor of shape \[F,3\]"):
                call(f=bad)
        for bad in (torch.zeros(6, dtype=torch.bool), torch.zeros(8, dtype=torch.bool), torch.zeros(7, 1, dtype=torch.bool), torch.zeros(7, dtype=torch.uint8), torch.zeros(7)):
            with pytest.raises(RuntimeError, match=r"as a bool tensor of shape \[F\] = \[7\]"):            # a selection or a hit of the wrong length or type
                call(s=bad)
        with pytest.raises(RuntimeError, match="num_vertices must be >= 0"):
            call(V=-1)
        with pytest.raises(RuntimeError, match=f"youreditableavatar_amd.mesh_region has no CPU path: faces must be on a HIP device"):
            call()
    for name in ("dilate_faces", "erode_faces"):
        for bad in (-1, 1.5, (1 << 20) + 1, None, True):
            with pytest.raises(RuntimeError, match=r"iterations is an int in \[0, 2\^20\]"):
                calls[name](iterations=bad)
    for kw in (dict(dilate_iter=-1), dict(erode_iter=-1), dict(dilate_iter=2.0), dict(erode_iter=(1 << 20) + 1)):
        with pytest.raises(RuntimeError, match=r"_iter is an int in \[0, 2\^20\]"):
            mr.refine_region(faces, sel, 10, **kw)
    with pytest.raises(RuntimeError, match="has no CPU path"):
        mr.refine_region(faces, torch.tensor([0, 3], dtype=torch.int64), 10)   # an index tensor is a legal hit
    assert mr.Region._fields == ("face_mask", "vertex_mask")


def test_the_docs_have_the_region_edits():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 4r"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd import mesh_region", "back_project", "dr.hit_faces", "refine_region", "mask_dilate = (~region.vertex_mask).float()[:, None]",
                 "verts_mask &= ~region.vertex_mask", "faces_mask", "editing_mask", "editing_mask_faces", "keep_large_components", "by coordinates", "goes by index",
                 "remove_duplicate_faces", "pymeshlab", "open3d", "(2, 5)", "(8, 10)"):
        assert what in sec, what
    assert "mesh_region" in open(os.path.join(ROOT, "README.md")).read() and "mesh_region" in open(os.path.join(ROOT, "DESIGN.md")).read()
