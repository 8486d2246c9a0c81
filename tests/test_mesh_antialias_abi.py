"""CPU: antialias and the topology build at the C ABI and in youreditableavatar_amd.mesh_raster_aa (no device needed): the header declares and
the cross-compiled library exports the four entry points, the header states the rule, bad arguments are refused before any device call, and
the module refuses what it cannot serve."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_mesh_topology_workspace_bytes", "tgs_mesh_topology", "tgs_mesh_antialias_workspace_bytes", "tgs_mesh_antialias")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import _mesh
    lib = _mesh.declare(ctypes.CDLL(lib_path()))            # its own handle, the package's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_antialias_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_mesh_topology_workspace_bytes\(int F\);", src)
    assert re.search(r"int\s+tgs_mesh_topology\(void\* stream, int V, int F, const int32_t\* tri, int32_t\* topo, void\* workspace, size_t workspace_bytes\);", src)
    assert re.search(r"size_t\s+tgs_mesh_antialias_workspace_bytes\(int width, int height\);", src)
    assert re.search(r"int\s+tgs_mesh_antialias\(void\* stream, int V, int F, int C, const float\* pos, const int32_t\* tri, const int32_t\* topo,\s*"
                     r"int width, int height, const float\* rast, const float\* color, float\* out,\s*void\* workspace, size_t workspace_bytes\);", src)
    # behind the mesh rasterizer's block, and the rule's key phrases
    assert src.index("tgs_mesh_interpolate(") < src.index("tgs_mesh_topology_workspace_bytes(")
    block = text[text.index("mesh rasterizer: antialias"):]
    for rule in ("E_ab(P) = s [(Xb-Xa)(Py-Ya) - (Yb-Ya)(Px-Xa)]", "vertex k to vertex (k+1) mod 3", "opposite vertex", "more than one other",
                 "smaller rast.z", "the lower ID", "the first k in 0, 1, 2", "D = s [(Xb-Xa) uy - (Yb-Ya) ux] < 0", "0 <= E(P) <= -D",
                 "min(Ya,Yb) <= Py <= max(Ya,Yb)", "min(Xa,Xb) <= Px <= max(Xa,Xb)", "E_ab(o) >= 0", "t = E(P) / (-D)", "a = t - 0.5",
                 "a (color[P] - color[Q])", "(-a) (color[Q] - color[P])", "left neighbour, right, row below (j-1), row above", "No float atomics",
                 "out may not alias color", "2^62"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build
    assert "tgs_mesh_aa.hip" in build.SOURCES


def test_workspace_sizes():
    lib = _lib()
    tw, aw = lib.tgs_mesh_topology_workspace_bytes, lib.tgs_mesh_antialias_workspace_bytes
    assert tw(0) > 0 and tw(1000) >= 3 * 1000 * 20                  # a slot (8-byte key, count, min, max) for every edge at least
    assert tw(1 << 20) > tw(1000) and tw(1 << 20) <= (4 << 20) * 2 * 20 + 4096
    assert tw(-1) == 0 and tw(1 << 24) == 0 and tw((1 << 24) - 1) > 0
    assert aw(1, 1) > 0 and aw(256, 256) >= 256 * 256 * 8 and aw(2048, 2048) <= 2048 * 2048 * 8 + 4096
    assert aw(512, 256) > aw(256, 256)
    for bad in ((0, 16), (16, -2), (8193, 16), (16, 8193)):
        assert aw(*bad) == 0, bad


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    tbig = lib.tgs_mesh_topology_workspace_bytes(10)

    def topo(V=8, F=10, tri=some, out=some, ws=some, nbytes=tbig):
        return lib.tgs_mesh_topology(None, V, F, tri, out, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(tri=None), dict(out=None), dict(ws=None), dict(nbytes=tbig - 1), dict(nbytes=0)):
        assert topo(**kw) == INVALID and "tgs_mesh_topology" in msg(), (kw, msg())
    assert topo(F=0, tri=None, out=None) == 0                      # no faces: nothing is launched, nothing written

    abig = lib.tgs_mesh_antialias_workspace_bytes(64, 48)

    def aa(V=8, F=10, C=3, pos=some, tri=some, topo=some, W=64, H=48, rast=some, color=some, out=other, ws=some, nbytes=abig):
        return lib.tgs_mesh_antialias(None, V, F, C, pos, tri, topo, W, H, rast, color, out, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(C=0), dict(C=-2), dict(W=0), dict(H=-3), dict(W=8193), dict(H=8193), dict(pos=None), dict(tri=None),
               dict(topo=None), dict(rast=None), dict(color=None), dict(out=None), dict(ws=None), dict(nbytes=abig - 1), dict(nbytes=0), dict(out=some),
               dict(W=8192, H=8192, C=1 << 14, nbytes=lib.tgs_mesh_antialias_workspace_bytes(8192, 8192))):
        assert aa(**kw) == INVALID and "tgs_mesh_antialias" in msg(), (kw, msg())
    assert aa(out=some) == INVALID and "alias" in msg()


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_raster as base
    import youreditableavatar_amd.mesh_raster_aa as dr
    for name in ("RasterizeCudaContext", "rasterize", "interpolate", "face_ids", "hit_faces"):
        assert getattr(dr, name) is getattr(base, name), name     # re-exported unchanged
    assert callable(dr.antialias) and callable(dr.antialias_construct_topology_hash)
    pos, tri = torch.zeros(1, 3, 4), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rast, color = torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 2)
    topo = torch.full((1, 3), -1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dr.antialias(color, rast, pos, tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dr.antialias(color, rast, pos[0], tri, topology_hash=topo, pos_gradient_boost=3.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dr.antialias_construct_topology_hash(tri)
    # wrong dtype or shape
    for bad_color in (color.double(), torch.zeros(4, 4, 2), torch.zeros(1, 4, 5, 2), torch.zeros(2, 4, 4, 2), torch.zeros(1, 4, 4, 0)):
        with pytest.raises(RuntimeError, match="color"):
            dr.antialias(bad_color, rast, pos, tri)
    for bad_rast in (rast.double(), torch.zeros(4, 4, 4), torch.zeros(1, 4, 4, 3)):
        with pytest.raises(RuntimeError, match="rast"):
            dr.antialias(color, bad_rast, pos, tri)
    for bad_pos in (pos.double(), torch.zeros(3, 3), torch.zeros(1, 1, 3, 4), torch.zeros(2, 3, 4)):
        with pytest.raises(RuntimeError, match="pos"):
            dr.antialias(color, rast, bad_pos, tri)
    for bad_tri in (tri.long(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="tri"):
            dr.antialias(color, rast, pos, bad_tri)
        with pytest.raises(RuntimeError, match="tri"):
            dr.antialias_construct_topology_hash(bad_tri)
    for bad_topo in (topo.long(), topo.float(), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), [[-1, -1, -1]]):
        with pytest.raises(RuntimeError, match="topology"):
            dr.antialias(color, rast, pos, tri, topology_hash=bad_topo)
    # forward only: an input that requires a gradient is refused, not detached -- and that is said before the device is
    for kw in (dict(color=color.clone().requires_grad_(True)), dict(rast=rast.clone().requires_grad_(True)), dict(pos=pos.clone().requires_grad_(True))):
        args = dict(color=color, rast=rast, pos=pos)
        args.update(kw)
        with pytest.raises(RuntimeError, match="forward only"):
            dr.antialias(args["color"], args["rast"], args["pos"], tri)
    # shape and dtype come first
    with pytest.raises(RuntimeError, match="topology"):
        dr.antialias(color.clone().requires_grad_(True), rast, pos, tri, topology_hash=topo.long())
    too_many = torch.zeros(1, 3, dtype=torch.int32).expand(1 << 24, 3)
    with pytest.raises(RuntimeError, match="2\\^24"):
        dr.antialias(color, rast, pos, too_many)
    with pytest.raises(RuntimeError, match="2\\^24"):
        dr.antialias_construct_topology_hash(too_many)


def test_the_docs_have_the_antialias_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4k" in text and text.index("## 4j") < text.index("## 4k") < text.index("## 5. ")
    sec = text[text.index("## 4k"):text.index("## 5. ")]
    for what in ("import youreditableavatar_amd.mesh_raster_aa as dr", "five edits", "not needed", "exit edge", "extent", "integer", "fixed order",
                 "float atomics", "gradients", "rast_db", "clipping", "eta_aa", "antialias_construct_topology_hash", "tools/mesh_antialias_loop.py"):
        assert what in sec, what
    for doc, what in (("README.md", "mesh_raster_aa"), ("SURVEY.md", "4k"), ("DESIGN.md", "tgs_mesh_aa.hip")):
        assert what in open(os.path.join(ROOT, doc)).read(), (doc, what)
