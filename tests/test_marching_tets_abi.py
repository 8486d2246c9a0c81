"""CPU: marching tetrahedra at the C ABI and in youreditableavatar_amd.marching_tets (no device needed): the header declares and the
cross-compiled library exports the entry points, the header states the rules, the kernel's case table is the restatement's, the workspace sizes
are sane, bad arguments are refused before any device call, and the module refuses what it cannot serve, with messages."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import mt_ref as R
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
KERNELS = os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_marching_tets.hip")
NEW = ("tgs_marching_tets_workspace_bytes", "tgs_marching_tets_table_bytes", "tgs_marching_tets_classify", "tgs_marching_tets_edges", "tgs_marching_tets_emit",
       "tgs_marching_tets_backward_workspace_bytes", "tgs_marching_tets_backward")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import marching_tets
    lib = marching_tets.declare(ctypes.CDLL(lib_path()))     # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_marching_tets_workspace_bytes\(int N, int F\);", src)
    assert src.index("tgs_mesh_antialias_backward(") < src.index("tgs_marching_tets_workspace_bytes(")
    assert text.index("mesh rasterizer: gradients") < text.index("---- marching tetrahedra ----")
    block = text[text.index("---- marching tetrahedra ----"):]
    block = block[:block.index("tgs_marching_tets_backward(")]
    for rule in ("occ = sdf > 0", "a NaN counts as outside and an exact zero counts as outside", "one to three of the tetrahedron's corners are inside", "sum_k occ_k 2^k",
                 "exactly one endpoint inside", "(min index, max index)", "ascending lexicographic order", "never a\n *                crossing edge",
                 "Duplicated tetrahedra are legal", "w_a = (-sdf[b]) / D", "no contraction", "nothing cancels", "A NaN sdf on a crossing edge gives a NaN vertex",
                 "the one-triangle tetrahedra first", "two triangles adjacent", "(0,1) (0,2) (0,3) (1,2) (1,3) (2,3)", "prefix sum", "the hash only dedupes",
                 "No float atomics anywhere", "two runs give the same bits", "bitmap of N / 8 bytes", "First read-back", "Second read-back", "counts[2] != 0",
                 "TGS_ERR_INVALID", "nothing faults", "never from the 4 F worst case", "allocate nothing", "N, F < 2^31", "16-byte aligned", "one emit per edges call", "quadratic in the number of crossing edges", "dv/dsdf[a] = (pos[b] - v) / D",
                 "dv/dsdf[b] = (v - pos[a]) / D", "dv/dpos[a] = -sdf[b] / D", "gather per grid row", "no float atomics on gradient memory", "offsets of their own",
                 "rounded to fp32 once", "stored, not\n * accumulated", "exact zeros"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, marching_tets
    assert "tgs_marching_tets.hip" in build.SOURCES
    assert set(marching_tets.SIGNATURES) == set(NEW)
    for name, (_, argtypes) in marching_tets.SIGNATURES.items():             # the table has as many arguments as the header's declaration
        decl = re.search(name + r"\(([^;]*)\);", src).group(1)
        assert len(argtypes) == len(decl.split(",")), name


def test_the_kernels_case_table_is_the_restatements():
    """the table is written twice, in two notations: corner pairs as bytes in the kernel, as text in tests/mt_ref.py (which the fixture pins)"""
    text = open(KERNELS).read()
    body = text[text.index("MT_CASES[16] = {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("};")])
    rows = re.findall(r"(0ull|MT_ONE\([^)]*\)|MT_TWO\([^)]*\))", body)
    assert len(rows) == 16
    for code, (row, want) in enumerate(zip(rows, R.CASES)):
        corners = re.findall(r"0x([0-3])([0-3])", row) if row != "0ull" else []
        assert ["".join(c) for c in corners] == want.replace("|", " ").split(), code
        assert all(int(i) < int(j) and (code >> int(i) & 1) != (code >> int(j) & 1) for i, j in corners), code      # every corner is a crossing edge


def test_workspace_sizes():
    lib = _lib()
    ws, table, back = lib.tgs_marching_tets_workspace_bytes, lib.tgs_marching_tets_table_bytes, lib.tgs_marching_tets_backward_workspace_bytes
    assert ws(0, 0) > 0 and table(0) > 0 and back(0, 0) > 0
    N, F = 35937, 196608
    assert N // 8 + F + 4 * N <= ws(N, F) <= N // 8 + F + 4 * N + 2 * 4 * (F // 256) + 16384           # the bitmap, a byte per tetrahedron, a word per vertex
    assert ws(2 * N, F) > ws(N, F) and ws(N, 2 * F) > ws(N, F)
    assert 16 * 40000 <= table(40000) <= 32 * 40000 + 1024                                               # load between 1/4 and 1/2, 8 bytes a key
    assert table(3 * 100_000_000 // 50) < 256 << 20                                                      # 10^8 tetrahedra, 2 % on the surface: not hundreds of MB
    assert 8 * N + 4 * 8260 <= back(N, 8260) <= 8 * N + 4 * 8260 + 8192
    for bad in ((-1, 8), (8, -1)):
        assert ws(*bad) == 0, bad
    assert table(-1) == 0 and table(1 << 34) == 0 and back(-1, 4) == 0 and back(4, -1) == 0


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    N, F = 100, 300
    big, tbig = lib.tgs_marching_tets_workspace_bytes(N, F), lib.tgs_marching_tets_table_bytes(3 * 10 + 4 * 5)

    def classify(N=N, F=F, sdf=some, tet=some, is64=1, valid=some, counts=other, ws=some, nbytes=big):
        return lib.tgs_marching_tets_classify(None, N, F, sdf, tet, is64, valid, counts, ws, nbytes)
    odd = ctypes.c_void_p(4096 + 8)                                # a tet that is not 16-byte aligned
    for kw in (dict(N=-1), dict(F=-1), dict(sdf=None), dict(tet=None), dict(tet=odd), dict(is64=2), dict(is64=-1), dict(valid=None), dict(counts=None), dict(ws=None), dict(nbytes=big - 1),
               dict(nbytes=0)):
        assert classify(**kw) == INVALID and "tgs_marching_tets_classify" in msg(), (kw, msg())

    def edges(N=N, F=F, tet=some, is64=0, n_one=10, n_two=5, counts=other, ws=some, nbytes=big, table=some, tbytes=tbig):
        return lib.tgs_marching_tets_edges(None, N, F, tet, is64, n_one, n_two, counts, ws, nbytes, table, tbytes)
    for kw in (dict(N=0), dict(N=-1), dict(F=0), dict(tet=None), dict(tet=odd), dict(is64=3), dict(n_one=-1), dict(n_two=-1), dict(n_one=0, n_two=0), dict(n_one=200, n_two=101), dict(counts=None),
               dict(ws=None), dict(nbytes=big - 1), dict(table=None), dict(tbytes=tbig - 1), dict(tbytes=0)):
        assert edges(**kw) == INVALID and "tgs_marching_tets_edges" in msg(), (kw, msg())

    def emit(N=N, F=F, pos=some, sdf=some, tet=some, is64=1, n_one=10, n_two=5, M=40, verts=other, iv=other, faces=other, f2t=other, ws=some, nbytes=big, table=some, tbytes=tbig):
        return lib.tgs_marching_tets_emit(None, N, F, pos, sdf, tet, is64, n_one, n_two, M, verts, iv, faces, f2t, ws, nbytes, table, tbytes)
    for kw in (dict(N=0), dict(F=-2), dict(pos=None), dict(sdf=None), dict(tet=None), dict(tet=odd), dict(is64=2), dict(n_one=-1), dict(n_one=0, n_two=0), dict(n_two=400), dict(M=0), dict(M=-1),
               dict(M=51), dict(verts=None), dict(iv=None), dict(faces=None), dict(f2t=None), dict(ws=None), dict(nbytes=big - 1), dict(table=None), dict(tbytes=tbig - 1)):
        assert emit(**kw) == INVALID and "tgs_marching_tets_emit" in msg(), (kw, msg())

    bbig = lib.tgs_marching_tets_backward_workspace_bytes(N, 40)

    def backward(N=N, M=40, pos=some, sdf=some, iv=some, g=some, d_pos=other, d_sdf=other, ws=some, nbytes=bbig):
        return lib.tgs_marching_tets_backward(None, N, M, pos, sdf, iv, g, d_pos, d_sdf, ws, nbytes)
    for kw in (dict(N=-1), dict(M=-1), dict(N=0), dict(pos=None), dict(sdf=None), dict(iv=None), dict(g=None), dict(ws=None), dict(nbytes=bbig - 1), dict(nbytes=0)):
        assert backward(**kw) == INVALID and "tgs_marching_tets_backward" in msg(), (kw, msg())
    assert backward(d_pos=None, d_sdf=None) == 0                  # no gradient wanted: nothing launched
    assert backward(N=0, M=0, pos=None, sdf=None, iv=None, g=None, d_pos=None, d_sdf=None) == 0


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.marching_tets as mt
    assert "no CPU path" in mt.__doc__ and "read" in mt.__doc__ and "call shape" in mt.marching_tetrahedra.__doc__ + mt.__doc__
    pos, sdf, tet = torch.zeros(5, 3), torch.zeros(5), torch.zeros(2, 4, dtype=torch.int64)
    grad = lambda t: t.clone().requires_grad_(True)
    for p, s in ((pos, sdf), (grad(pos), sdf), (pos, grad(sdf))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            mt.marching_tets(p, s, tet)
        with pytest.raises(RuntimeError, match="no CPU path"):
            mt.marching_tets(p, s[:, None], tet.int())
        with pytest.raises(RuntimeError, match="float32 pos of shape"):
            mt.marching_tets(p.double(), s, tet)
        with pytest.raises(RuntimeError, match="float32 pos of shape"):
            mt.marching_tets(p[:, :2], s, tet)
        with pytest.raises(RuntimeError, match=r"float32 sdf of shape \[5\] or \[5,1\]"):
            mt.marching_tets(p, s[:4], tet)
        with pytest.raises(RuntimeError, match="float32 sdf"):
            mt.marching_tets(p, s.double(), tet)
        with pytest.raises(RuntimeError, match="int32 or int64 tet of shape"):
            mt.marching_tets(p, s, tet.short())
        with pytest.raises(RuntimeError, match="int32 or int64 tet of shape"):
            mt.marching_tets(p, s, tet[:, :3])
    with pytest.raises(RuntimeError, match="must be a tensor"):
        mt.marching_tets(pos, sdf, [[0, 1, 2, 3]])
    with pytest.raises(RuntimeError, match=r"vertices of shape \[B,N,3\]"):
        mt.marching_tetrahedra(pos, tet, sdf)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mt.marching_tetrahedra(pos[None], tet, sdf[None], return_tet_idx=True)


def test_the_docs_have_the_isosurface_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4m" in text and text.index("## 4l") < text.index("## 4m") < text.index("## 5. ")
    sec = text[text.index("## 4m"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.marching_tets import marching_tets", "marching_tetrahedra", "read-back", "NaN", "outside [0, N)", "[M,1,2]", "eta",
                 "tools/marching_tets_loop.py", "examples/fit_sdf_silhouette.py", "Measured", "not measured"):
        assert what in sec, what
    assert "marching_tets" in open(os.path.join(ROOT, "README.md")).read()
    assert "marching_tets" in open(os.path.join(ROOT, "SURVEY.md")).read()
