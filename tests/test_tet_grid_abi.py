"""CPU: the tetrahedral grid's passes at the C ABI and in youreditableavatar_amd.tet_grid (no device needed): the header declares and the
cross-compiled library exports the entry points, the header states the rules, the signature table matches the header, the shared pieces live in
their headers, the workspace sizes are sane, bad arguments are refused before any device call, and the module refuses what it cannot serve."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
CSRC = os.path.join(ROOT, "youreditableavatar_amd", "csrc")
NEW = ("tgs_tet_compact_workspace_bytes", "tgs_tet_compact_select", "tgs_tet_compact_emit", "tgs_tet_subdivide_workspace_bytes", "tgs_tet_subdivide_edges", "tgs_tet_subdivide_emit")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import tet_grid
    lib = tet_grid.declare(ctypes.CDLL(lib_path()))          # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_tet_compact_workspace_bytes\(int N, int F\);", src)
    assert src.index("tgs_hashgrid_field_backward(") < src.index("tgs_tet_compact_workspace_bytes(")           # behind the hash-grid block
    assert text.index("---- hash-grid field ----") < text.index("---- tetrahedral grids ----")
    block = text[text.index("---- tetrahedral grids ----"):]
    block = block[:block.index("tgs_tet_subdivide_emit(")]
    for rule in ("fabsf((((s0 + s1) + s2) + s3) * 0.25f) <= threshold", "left to\n *                right", "no contraction", "A NaN mean is dropped", "keep[F]",
                 "ascending", "rank of tet[old, k] in unique_vtx", "bit copies", "membership by index", "atomicOr", "popcount", "counts[2] != 0", "nothing faults",
                 "The one read-back", "ab, ac, ad, bc, bd, cd", "(min index, max index)", "ascending lexicographic order", "An edge (v, v)", "listed twice adds nothing",
                 "(pos[e0] + pos[e1]) * 0.5f", "A non-finite input propagates", "sum to 2", "row k F + f", "(a, ab, ac, ad)", "(b, bc, ab, bd)", "(c, ac, bc, cd)", "(d, ad, cd, bd)",
                 "(ab, ac, ad, bd)", "(ab, ac, bd, bc)", "(cd, ac, bd, ad)", "(cd, ac, bc, bd)", "sub_to_parent[k F + f] = f", "no hash table", "24 bytes of workspace per tetrahedron",
                 "N + E < 2^31", "(2^31 - 1) / 8", "16-byte aligned", "allocate nothing", "No float atomics anywhere", "two runs give the same bits", "TGS_ERR_INVALID"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, tet_grid
    assert "tgs_tet_grid.hip" in build.SOURCES
    assert set(tet_grid.SIGNATURES) == set(NEW)
    for name, (_, argtypes) in tet_grid.SIGNATURES.items():                  # the table has as many arguments as the header's declaration, floats where it has floats
        decl = re.search(name + r"\(([^;]*)\);", src).group(1).split(",")
        assert len(argtypes) == len(decl), name
        for a, d in zip(argtypes, decl):
            want = ctypes.c_void_p if "*" in d else ctypes.c_float if "float" in d else ctypes.c_int64 if "int64_t" in d else ctypes.c_size_t if "size_t" in d else ctypes.c_int
            assert a is want, (name, d.strip())


def test_the_shared_pieces_have_one_copy():
    """the scans, the run bounds, the run sort and the binary search: tgs_runs.hpp; the edge set, its fill and its sort: tgs_edge_set.hpp; the row
    load: tgs_tet_common.hpp.  Each definition stands once, in its header, and in none of the four kernel files of the geometry stage"""
    read = lambda name: open(os.path.join(CSRC, name)).read()
    shared = {
        "tgs_runs.hpp": ("size_t run_scan_scratch(", "size_t run_blocks(", "dim3 run_grid(", "uint32_t run_block_escan(", "void k_run_scan_sums(", "void k_run_scan_tile(",
                         "void run_scan(", "size_t run_start(", "Run run_bounds(", "void run_sort(", "long long run_sort_unique(", "long long run_search("),
        "tgs_edge_set.hpp": ("EDGE_EMPTY = ", "unsigned long long edge_key(", "unsigned long long edge_hash(", "0xbf58476d1ce4e5b9ull", "size_t edge_insert(", "size_t edge_find(",
                             "void k_edge_fill(", "void k_edge_sort("),
        "tgs_tet_common.hpp": ("void mt_load_tet(", "bool mt_in_range(", "bool mt_aligned("),
    }
    kernel_files = {name: read(name) for name in ("tgs_marching_tets.hip", "tgs_tet_grid.hip", "tgs_mesh_geom.hip", "tgs_mesh_aa.hip")}
    for header, definitions in shared.items():
        text = read(header)
        assert text.count("__global__") == text.count("static __global__"), header    # a kernel in a header is static: one copy per translation unit, no relocatable device code
        for once in definitions:
            assert text.count(once) == 1, (header, once)
            for other, code in {**{h: read(h) for h in set(shared) - {header}}, **kernel_files}.items():
                assert once not in code, (other, once)
    assert '#include "tgs_runs.hpp"' in read("tgs_tet_common.hpp") and '#include "tgs_runs.hpp"' in read("tgs_edge_set.hpp")
    includes = {"tgs_marching_tets.hip": ("tgs_tet_common.hpp", "tgs_edge_set.hpp"), "tgs_tet_grid.hip": ("tgs_tet_common.hpp",), "tgs_mesh_geom.hip": ("tgs_edge_set.hpp",),
                "tgs_mesh_aa.hip": ("tgs_edge_set.hpp",)}
    for source, text in kernel_files.items():
        for header in includes[source]:
            assert f'#include "{header}"' in text, (source, header)
        assert "atomicCAS" not in text, source                               # the probe loop is the edge set's
        for old in ("mt_scan", "mg_scan", "_block_escan(uint32_t", "mt_sort_run", "mt_sort_unique_run", "mt_search_run", "mg_run(", "mg_hash", "mt_hash", "topo_hash", "k_mg_edge_fill",
                    "k_mg_edge_sort", "k_mt_fill", "k_mt_sort_runs", "MT_EMPTY", "MG_EMPTY", "TOPO_EMPTY", "end[v - 1]", "run[v - 1]", "run[a - 1]", "run_b[v - 1]"):
            assert old not in text, (source, old)
        for float_atomic in ("atomicAdd(float", "unsafeAtomicAdd", "atomicAdd_system"):
            assert float_atomic not in text, (source, float_atomic)
    assert "atomicCAS" in read("tgs_edge_set.hpp")
    for source in ("tgs_marching_tets.hip", "tgs_mesh_geom.hip"):
        text = kernel_files[source]
        assert "edge_insert(" in text and "k_edge_fill," in text and "k_edge_sort," in text and "run_scan(" in text and "run_bounds(" in text and "run_sort(" in text, source
    aa, grid = kernel_files["tgs_mesh_aa.hip"], kernel_files["tgs_tet_grid.hip"]
    assert "edge_insert(" in aa and "edge_find(" in aa and "edge_key(" in aa
    assert "run_search(" in kernel_files["tgs_marching_tets.hip"]
    assert "run_sort_unique(" in grid and "run_search(" in grid and "run_scan(" in grid and "run_bounds(" in grid and "run_start(" in grid
    assert "tgs_edge_set.hpp" not in grid and "edge_insert" not in grid and "edge_find" not in grid                # the subdivision has no hash table


def test_workspace_sizes():
    lib = _lib()
    compact, subdiv = lib.tgs_tet_compact_workspace_bytes, lib.tgs_tet_subdivide_workspace_bytes
    assert compact(0, 0) > 0 and subdiv(0, 0) > 0
    N, F = 35937, 196608
    assert N // 8 + F + 4 * (N // 64) <= compact(N, F) <= N // 8 + F + 4 * (N // 64) + 4 * (F // 256) + 16384   # the bitmap, a byte per tetrahedron, a word per bitmap word
    assert 24 * F + 8 * N <= subdiv(N, F) <= 24 * F + 8 * N + 16384                                           # 24 bytes per tetrahedron, two words per vertex
    assert compact(2 * N, F) > compact(N, F) and compact(N, 2 * F) > compact(N, F) and subdiv(2 * N, F) > subdiv(N, F) and subdiv(N, 2 * F) > subdiv(N, F)
    for bad in ((-1, 8), (8, -1)):
        assert compact(*bad) == 0 and subdiv(*bad) == 0, bad
    assert subdiv(8, ((1 << 31) - 1) // 8) > 0 and subdiv(8, ((1 << 31) - 1) // 8 + 1) == 0                    # 8 F rows stay below 2^31


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    odd = ctypes.c_void_p(4096 + 8)                                # a tet that is not 16-byte aligned
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    N, F = 100, 300
    cbig, sbig = lib.tgs_tet_compact_workspace_bytes(N, F), lib.tgs_tet_subdivide_workspace_bytes(N, F)

    def select(N=N, F=F, sdf=some, tet=some, is64=1, keep=None, thr=0.02, counts=other, ws=some, nbytes=cbig):
        return lib.tgs_tet_compact_select(None, N, F, sdf, tet, is64, keep, thr, counts, ws, nbytes)
    for kw in (dict(N=-1), dict(F=-1), dict(sdf=None), dict(tet=None), dict(tet=odd), dict(is64=2), dict(is64=-1), dict(counts=None), dict(ws=None), dict(nbytes=cbig - 1), dict(nbytes=0)):
        assert select(**kw) == INVALID and "tgs_tet_compact_select" in msg(), (kw, msg())

    def emit(N=N, F=F, tet=some, is64=0, n_tets=10, n_verts=20, pos=some, sdf=some, mask=None, mtype=0, member_ws=None, out64=1, new_tets=other, to_old=other, vtx=other,
             new_pos=other, new_sdf=other, new_mask=None, member=None, ws=some, nbytes=cbig):
        return lib.tgs_tet_compact_emit(None, N, F, tet, is64, n_tets, n_verts, pos, sdf, mask, mtype, member_ws, out64, new_tets, to_old, vtx, new_pos, new_sdf, new_mask, member, ws, nbytes)
    for kw in (dict(N=0), dict(F=0), dict(F=-3), dict(tet=None), dict(tet=odd), dict(is64=2), dict(out64=2), dict(n_tets=0), dict(n_tets=301), dict(n_verts=0), dict(n_verts=101),
               dict(n_tets=2, n_verts=9), dict(new_tets=None), dict(to_old=None), dict(vtx=None), dict(new_pos=None), dict(new_sdf=None), dict(mask=some), dict(mask=some, new_mask=other, mtype=4),
               dict(mtype=-1), dict(member_ws=some), dict(ws=None), dict(nbytes=cbig - 1), dict(nbytes=0)):
        assert emit(**kw) == INVALID and "tgs_tet_compact_emit" in msg(), (kw, msg())

    def edges(N=N, F=F, tet=some, is64=1, counts=other, ws=some, nbytes=sbig):
        return lib.tgs_tet_subdivide_edges(None, N, F, tet, is64, counts, ws, nbytes)
    for kw in (dict(N=-1), dict(F=-1), dict(tet=None), dict(tet=odd), dict(is64=2), dict(counts=None), dict(ws=None), dict(nbytes=sbig - 1), dict(nbytes=0)):
        assert edges(**kw) == INVALID and "tgs_tet_subdivide_edges" in msg(), (kw, msg())
    assert lib.tgs_tet_subdivide_edges(None, 8, ((1 << 31) - 1) // 8 + 1, some, 1, other, some, 1 << 40) == INVALID and "tgs_tet_subdivide_edges" in msg()

    def semit(N=N, F=F, B=1, E=500, pos=some, tet=some, is64=1, mask=None, mtype=0, new_v=other, new_tets=other, new_mask=None, sub=other, ed=other, ws=some, nbytes=sbig):
        return lib.tgs_tet_subdivide_emit(None, N, F, B, E, pos, tet, is64, mask, mtype, new_v, new_tets, new_mask, sub, ed, ws, nbytes)
    for kw in (dict(N=0), dict(F=0), dict(B=-1), dict(B=65536), dict(E=0), dict(E=-1), dict(E=1801), dict(pos=None), dict(tet=None), dict(tet=odd), dict(is64=2), dict(mask=some),
               dict(mtype=4), dict(new_v=None), dict(new_tets=None), dict(sub=None), dict(ed=None), dict(ws=None), dict(nbytes=sbig - 1), dict(nbytes=0)):
        assert semit(**kw) == INVALID and "tgs_tet_subdivide_emit" in msg(), (kw, msg())
    huge_n, many = (1 << 31) - 600, 200                            # N + E at 2^31: refused (the workspace size is checked after the counts)
    assert lib.tgs_tet_subdivide_emit(None, huge_n, many, 1, 600, some, some, 1, None, 0, other, other, None, other, other, some, 1 << 40) == INVALID and "tgs_tet_subdivide_emit" in msg()


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.tet_grid as tg
    assert "no CPU path" in tg.__doc__ and "read" in tg.__doc__ and "framework's arithmetic" in tg.subdivide_tets.__doc__
    assert "vertex index" in tg.mark_part_tets.__doc__ and "no two grid vertices share a position" in tg.mark_part_tets.__doc__.replace("\n    ", " ")
    pos, sdf, tet = torch.zeros(5, 3), torch.zeros(5), torch.zeros(2, 4, dtype=torch.int64)
    mask = torch.zeros(5, 1, dtype=torch.int32)
    for call in (lambda: tg.compact_tets(pos, sdf, tet), lambda: tg.compact_tets(pos, sdf[:, None], tet.int(), mask), lambda: tg.subdivide_tets(pos, tet),
                 lambda: tg.subdivide_tets(pos.clone().requires_grad_(True), tet, mask), lambda: tg.batch_subdivide_volume(pos[None], tet[None], mask[None]),
                 lambda: tg.mark_part_tets(pos, sdf[:, None], tet, torch.zeros(0, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="float32 pos of shape"):
        tg.compact_tets(pos.double(), sdf, tet)
    with pytest.raises(RuntimeError, match="float32 pos of shape"):
        tg.subdivide_tets(pos[:, :2], tet)
    with pytest.raises(RuntimeError, match=r"float32 sdf of shape \[5\] or \[5,1\]"):
        tg.compact_tets(pos, sdf[:4], tet)
    with pytest.raises(RuntimeError, match="int32 or int64 tet of shape"):
        tg.compact_tets(pos, sdf, tet.short())
    with pytest.raises(RuntimeError, match="int32 or int64 tet of shape"):
        tg.subdivide_tets(pos, tet[:, :3])
    with pytest.raises(RuntimeError, match=r"mask of shape \[5\] or \[5,1\]"):
        tg.compact_tets(pos, sdf, tet, mask[:4])
    with pytest.raises(RuntimeError, match="one-byte mask"):
        tg.subdivide_tets(pos, tet, mask.double())
    with pytest.raises(RuntimeError, match="must be a tensor"):
        tg.compact_tets(pos, sdf, [[0, 1, 2, 3]])
    with pytest.raises(RuntimeError, match=r"tet_bxfx4 of shape \[B,...,...\]"):
        tg.batch_subdivide_volume(pos[None], tet)
    with pytest.raises(RuntimeError, match=r"mask_keep_part_in_new_pos of shape \[1,5,1\]"):
        tg.batch_subdivide_volume(pos[None], tet[None], mask[None, :4])


def test_the_docs_have_the_tetrahedral_grid_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4p" in text and text.index("## 4o") < text.index("## 4p") < text.index("## 5. ")
    sec = text[text.index("## 4p"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.tet_grid import", "compact_tets", "batch_subdivide_volume", "mark_part_tets", "subdivide_tets", "read-back", "threshold", "index_dtype",
                 "edges", "vertex index", "tools/tet_grid_loop.py", "a record, not a bar", "Measured", "not measured", "per-kernel", "open-addressing"):
        assert what in sec, what
    assert "tet_grid" in open(os.path.join(ROOT, "README.md")).read()
    assert "tet_grid" in open(os.path.join(ROOT, "DESIGN.md")).read()
