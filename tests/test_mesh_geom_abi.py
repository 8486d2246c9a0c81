"""CPU: mesh geometry at the C ABI and in youreditableavatar_amd.mesh_geom (no device needed): the header declares and the cross-compiled library
exports the entry points, the header states the rules, the signature table matches the header, the workspace sizes are sane, bad arguments are
refused before any device call, and the module refuses what it cannot serve, with messages."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_meshgeom_workspace_bytes", "tgs_meshgeom_table_bytes", "tgs_meshgeom_normals_backward_workspace_bytes", "tgs_meshgeom_topology_count",
       "tgs_meshgeom_topology_fill", "tgs_meshgeom_normals", "tgs_meshgeom_normals_backward", "tgs_meshgeom_consistency", "tgs_meshgeom_consistency_backward",
       "tgs_meshgeom_laplacian", "tgs_meshgeom_laplacian_backward")
INVALID = -1
MAX_FACES = ((1 << 32) - 1) // 3


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import mesh_geom
    lib = mesh_geom.declare(ctypes.CDLL(lib_path()))         # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_meshgeom_workspace_bytes\(int V, int F\);", src)
    assert src.index("tgs_marching_tets_backward(") < src.index("tgs_meshgeom_workspace_bytes(")
    assert text.index("---- marching tetrahedra ----") < text.index("---- mesh geometry ----")
    block = text[text.index("---- mesh geometry ----"):]
    block = block[:block.index("tgs_meshgeom_laplacian_backward(")]
    for rule in ("3 * face + corner", "ascending lexicographic", "A pair (i, i)", "is kept", "max_list", "hold the ENDS of the runs", "the hash only dedupes", "sized from 3 F",
                 "counts[0] = E", "counts[1] != 0", "TGS_ERR_INVALID", "nothing faults", "read nothing back", "cross(v1 - v0, v2 - v0)", "always along the last axis",
                 "added in double in run order", "(0, 0, 1)", "> 1e-20", "a non-finite sum", "rounded to fp32 once", "F.normalize, safe_normalize", "g_s = (g - n (n . g)) / |s|",
                 "an exact zero for a", "e2 x G", "G x e1", "0 * NaN is a NaN", "Rows\n *                that no face touches are exact zeros", "max(|row|, 1e-8)", "fixed shuffle tree",
                 "in a fixed order", "min-end run, then its max-end list", "distinct neighbours o != v", "adds -1 and +1 to the diagonal", "zero subgradient", "the operator is symmetric",
                 "No float atomics anywhere", "no atomics at all on gradient memory", "two runs give the same bits", "stored,\n * not accumulated", "F <= (2^32 - 1) / 3",
                 "allocate nothing"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, mesh_geom
    assert "tgs_mesh_geom.hip" in build.SOURCES
    assert set(mesh_geom.SIGNATURES) == set(NEW)
    for name, (_, argtypes) in mesh_geom.SIGNATURES.items():                 # the table has as many arguments as the header's declaration
        decl = re.search(name + r"\(([^;]*)\);", src).group(1)
        assert len(argtypes) == len(decl.split(",")), name
        for ctype, arg in zip(argtypes, decl.split(",")):                    # and the same kinds: pointers, int, int64_t, size_t
            want = ctypes.c_void_p if "*" in arg else ctypes.c_int64 if "int64_t" in arg else ctypes.c_size_t if "size_t" in arg else ctypes.c_int
            assert ctype is want, (name, arg)


def test_workspace_sizes():
    lib = _lib()
    ws, table, back = lib.tgs_meshgeom_workspace_bytes, lib.tgs_meshgeom_table_bytes, lib.tgs_meshgeom_normals_backward_workspace_bytes
    assert ws(0, 0) > 0 and table(0) > 0 and back(0, 0) > 0
    V, F = 133544, 267084                                                    # the 128^3 grid's mesh
    assert 8 * (3 * F // 256) <= ws(V, F) <= 8 * (3 * F // 256) + 4 * (V // 2048) + 16384   # a double per workgroup of the losses, the scans' scratch
    assert ws(2 * V, F) >= ws(V, F) and ws(V, 2 * F) > ws(V, F)
    assert 8 * 6 * F <= table(F) <= 8 * 12 * F + 1024                          # load between 1/4 and 1/2, 8 bytes a key
    assert 24 * (V + F) <= back(V, F) <= 24 * (V + F) + 4096                   # a double row per vertex and per face
    for bad in ((-1, 8), (8, -1), (8, MAX_FACES + 1)):
        assert ws(*bad) == 0 and back(*bad) == 0, bad
    assert table(-1) == 0 and table(MAX_FACES + 1) == 0 and table(MAX_FACES) > 0


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    V, F, E = 100, 300, 450
    big, tbig, bbig = lib.tgs_meshgeom_workspace_bytes(V, F), lib.tgs_meshgeom_table_bytes(F), lib.tgs_meshgeom_normals_backward_workspace_bytes(V, F)

    def count(V=V, F=F, faces=some, is64=1, inc_end=other, edge_end=other, max_end=other, counts=other, table=some, tbytes=tbig, ws=some, nbytes=big):
        return lib.tgs_meshgeom_topology_count(None, V, F, faces, is64, inc_end, edge_end, max_end, counts, table, tbytes, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=0), dict(F=MAX_FACES + 1), dict(faces=None), dict(is64=2), dict(is64=-1), dict(inc_end=None), dict(edge_end=None), dict(max_end=None),
               dict(counts=None), dict(tbytes=tbig - 1), dict(tbytes=0), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0)):
        assert count(**kw) == INVALID and "tgs_meshgeom_topology_count" in msg(), (kw, msg())

    def fill(V=V, F=F, faces=some, is64=0, E=E, inc_end=other, inc=other, edge_end=other, max_end=other, edges=other, max_list=other, table=some, tbytes=tbig):
        return lib.tgs_meshgeom_topology_fill(None, V, F, faces, is64, E, inc_end, inc, edge_end, max_end, edges, max_list, table, tbytes)
    for kw in (dict(V=0), dict(V=-1), dict(F=0), dict(faces=None), dict(is64=3), dict(E=-1), dict(E=0), dict(E=3 * F + 1), dict(inc_end=None), dict(inc=None), dict(edge_end=None),
               dict(max_end=None), dict(edges=None), dict(max_list=None), dict(tbytes=tbig - 1), dict(table=None)):
        assert fill(**kw) == INVALID and "tgs_meshgeom_topology_fill" in msg(), (kw, msg())

    def normals(V=V, F=F, v_pos=some, faces=some, is64=1, inc_end=some, inc=some, out=other):
        return lib.tgs_meshgeom_normals(None, V, F, v_pos, faces, is64, inc_end, inc, out)
    for kw in (dict(V=-1), dict(F=-1), dict(F=MAX_FACES + 1), dict(v_pos=None), dict(faces=None), dict(is64=2), dict(inc_end=None), dict(inc=None), dict(out=None)):
        assert normals(**kw) == INVALID and "tgs_meshgeom_normals" in msg(), (kw, msg())
    assert normals(V=0, F=0, v_pos=None, faces=None, inc_end=None, inc=None, out=None) == 0

    def normals_bwd(V=V, F=F, v_pos=some, faces=some, is64=0, inc_end=some, inc=some, g=some, d_pos=other, ws=some, nbytes=bbig):
        return lib.tgs_meshgeom_normals_backward(None, V, F, v_pos, faces, is64, inc_end, inc, g, d_pos, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(v_pos=None), dict(faces=None), dict(is64=5), dict(inc_end=None), dict(inc=None), dict(g=None), dict(ws=None), dict(nbytes=bbig - 1), dict(nbytes=0)):
        assert normals_bwd(**kw) == INVALID and "tgs_meshgeom_normals_backward" in msg(), (kw, msg())
    assert normals_bwd(d_pos=None) == 0                           # no gradient wanted: nothing launched

    def consistency(V=V, E=E, v_nrm=some, edges=some, out=other, ws=some, nbytes=big):
        return lib.tgs_meshgeom_consistency(None, V, E, v_nrm, edges, out, ws, nbytes)
    for kw in (dict(V=0), dict(E=0), dict(E=-1), dict(E=1 << 32), dict(v_nrm=None), dict(edges=None), dict(out=None), dict(ws=None), dict(nbytes=0)):
        assert consistency(**kw) == INVALID and "tgs_meshgeom_consistency" in msg(), (kw, msg())

    def consistency_bwd(V=V, E=E, v_nrm=some, edges=some, edge_end=some, max_end=some, max_list=some, g=some, d_nrm=other):
        return lib.tgs_meshgeom_consistency_backward(None, V, E, v_nrm, edges, edge_end, max_end, max_list, g, d_nrm)
    for kw in (dict(V=0), dict(E=0), dict(v_nrm=None), dict(edges=None), dict(edge_end=None), dict(max_end=None), dict(max_list=None), dict(g=None)):
        assert consistency_bwd(**kw) == INVALID and "tgs_meshgeom_consistency_backward" in msg(), (kw, msg())
    assert consistency_bwd(d_nrm=None) == 0

    def laplacian(V=V, E=E, v_pos=some, edges=some, edge_end=some, max_end=some, max_list=some, unit=other, out=other, ws=some, nbytes=big):
        return lib.tgs_meshgeom_laplacian(None, V, E, v_pos, edges, edge_end, max_end, max_list, unit, out, ws, nbytes)
    for kw in (dict(V=0), dict(E=-1), dict(E=1 << 32), dict(v_pos=None), dict(edges=None), dict(edge_end=None), dict(max_end=None), dict(max_list=None), dict(out=None), dict(ws=None),
               dict(nbytes=0)):
        assert laplacian(**kw) == INVALID and "tgs_meshgeom_laplacian" in msg(), (kw, msg())

    def laplacian_bwd(V=V, E=E, edges=some, edge_end=some, max_end=some, max_list=some, unit=some, g=some, d_pos=other):
        return lib.tgs_meshgeom_laplacian_backward(None, V, E, edges, edge_end, max_end, max_list, unit, g, d_pos)
    for kw in (dict(V=0), dict(E=-1), dict(edges=None), dict(edge_end=None), dict(max_end=None), dict(max_list=None), dict(unit=None), dict(g=None)):
        assert laplacian_bwd(**kw) == INVALID and "tgs_meshgeom_laplacian_backward" in msg(), (kw, msg())
    assert laplacian_bwd(d_pos=None) == 0


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_geom as mg
    assert "no CPU path" in mg.__doc__ and "read-back" in mg.__doc__ and "exactly 3 faces" in mg.__doc__
    v, f = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int64)
    grad = lambda t: t.clone().requires_grad_(True)
    for p in (v, grad(v)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            mg.vertex_normals(p, f)
        with pytest.raises(RuntimeError, match="no CPU path"):
            mg.mesh_normal_consistency(p, f.int())
        with pytest.raises(RuntimeError, match=r"float32 v_pos of shape \[V,3\]"):
            mg.vertex_normals(p.double(), f)
        with pytest.raises(RuntimeError, match=r"float32 v_pos of shape \[V,3\]"):
            mg.vertex_normals(p[:, :2], f)
        with pytest.raises(RuntimeError, match="int32 or int64 faces of shape"):
            mg.vertex_normals(p, f.short())
        with pytest.raises(RuntimeError, match="int32 or int64 faces of shape"):
            mg.vertex_normals(p, torch.zeros(2, 4, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="must be a MeshTopology"):
            mg.laplacian(p, None)
        with pytest.raises(RuntimeError, match="must be a MeshTopology"):
            mg.normal_consistency(p, f)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        mg.vertex_normals(v, [[0, 1, 2]])
    with pytest.raises(RuntimeError, match="must be a tensor"):
        mg.mesh_topology([[0, 1, 2]], 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mg.mesh_topology(f, 5)
    for bad in (-1, 1 << 31, 2.5, None, True):
        with pytest.raises(RuntimeError, match="num_vertices must be an int"):
            mg.mesh_topology(f, bad)
    many = torch.zeros(1, 3, dtype=torch.int64).expand(MAX_FACES + 1, 3)     # (a view of one row: no memory)
    with pytest.raises(RuntimeError, match=r"at most \(2\^32 - 1\) / 3"):
        mg.mesh_topology(many, 5)
    with pytest.raises(RuntimeError, match=r"at most 2\^31 - 1"):
        mg.vertex_normals(torch.zeros(1, 3).expand(1 << 31, 3), f)
    here = torch.device("cpu")
    topo = mg.MeshTopology(5, 2, 0, here, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="built for 5 vertices and 2 faces"):
        mg._check_topology(topo, 6, 2, here, False)
    with pytest.raises(RuntimeError, match="built with edges=False"):
        mg._check_topology(topo, 5, None, here, True)


def test_the_docs_have_the_mesh_geometry_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4n" in text and text.index("## 4m") < text.index("## 4n") < text.index("## 5. ")
    sec = text[text.index("## 4n"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.mesh_geom import", "vertex_normals", "mesh_topology", "normal_consistency", "laplacian", "read-back", "NaN", "exactly 3 faces",
                 "eta", "tools/mesh_geom_loop.py", "examples/fit_sdf_normals.py", "Measured"):
        assert what in sec, what
    assert "mesh_geom" in open(os.path.join(ROOT, "README.md")).read()
    assert "mesh_geom" in open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "mesh_geom" in open(os.path.join(ROOT, "DESIGN.md")).read()
