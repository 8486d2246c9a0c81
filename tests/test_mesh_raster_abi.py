"""CPU: the mesh rasterizer at the C ABI and the public module (no device needed): the header declares and the cross-compiled library exports
the three entry points, bad arguments are refused before any device call, and youreditableavatar_amd.mesh_raster refuses what it cannot serve."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_mesh_workspace_bytes", "tgs_mesh_rasterize", "tgs_mesh_interpolate")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import _mesh
    lib = _mesh.declare(ctypes.CDLL(lib_path()))            # its own handle, the package's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_mesh_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_mesh_workspace_bytes\(int F, int width, int height\);", src)
    assert re.search(r"int\s+tgs_mesh_rasterize\(void\* stream, int V, int F, const float\* pos, const int32_t\* tri,\s*int width, int height, float\* rast, "
                     r"void\* workspace, size_t workspace_bytes\);", src)
    assert re.search(r"int\s+tgs_mesh_interpolate\(void\* stream, int V, int F, int C, const float\* attr, const int32_t\* tri,\s*int64_t n_pixels, "
                     r"const float\* rast, float\* out\);", src)
    for rule in ("rint((x/w * 0.5 + 0.5) * width * 256)", "dy < 0, or dy = 0 and dx > 0", "lower triangle index", "max(u + v, 1)", "2^29"):
        assert rule in text, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build
    assert "tgs_mesh.hip" in build.SOURCES


def test_the_signature_table_agrees_with_the_header():
    """every tgs_mesh_* prototype of the header, comments stripped: its return type and each parameter, in order, are the ctypes kinds of
    youreditableavatar_amd._mesh.SIGNATURES (any pointer a c_void_p), and the table names nothing the header lacks"""
    from youreditableavatar_amd import _mesh
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}

    def kind(decl):
        decl = decl.strip()
        if "*" in decl:
            return ctypes.c_void_p
        words = [w for w in decl.split() if w != "const"]
        return kinds[words[0]]                                     # (the type; a parameter's name follows it)
    protos = re.findall(r"([A-Za-z_0-9]+[\s\*]+)(tgs_mesh_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)
    declared = {name: (kind(ret), [kind(p) for p in params.split(",")]) for ret, name, params in protos}
    assert len(protos) == len(declared) == 11, sorted(declared)
    assert set(_mesh.SIGNATURES) == set(declared), set(_mesh.SIGNATURES) ^ set(declared)
    for name, (restype, argtypes) in declared.items():
        assert _mesh.SIGNATURES[name][0] is restype, name
        assert list(_mesh.SIGNATURES[name][1]) == argtypes, (name, _mesh.SIGNATURES[name][1], argtypes)


def test_workspace_size():
    lib = _lib()
    ws = lib.tgs_mesh_workspace_bytes
    assert ws(0, 1, 1) > 0
    assert ws(1000, 256, 256) >= 256 * 256 * 8 + 1000 * 12
    assert ws(1000, 512, 256) > ws(1000, 256, 256) and ws(2000, 256, 256) > ws(1000, 256, 256)
    assert ws(1 << 20, 2048, 2048) < 64 << 20                     # 8 bytes per pixel and 12 per face
    for bad in ((-1, 16, 16), (10, 0, 16), (10, 16, -2), (10, 8193, 16), (10, 16, 8193)):
        assert ws(*bad) == 0, bad


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some = ctypes.c_void_p(4096)            # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    big = lib.tgs_mesh_workspace_bytes(10, 64, 64)

    def rast(V=8, F=10, pos=some, tri=some, W=64, H=64, out=some, ws=some, nbytes=big):
        return lib.tgs_mesh_rasterize(None, V, F, pos, tri, W, H, out, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(W=0), dict(H=-3), dict(W=8193), dict(H=8193), dict(pos=None), dict(tri=None), dict(out=None),
               dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0)):
        assert rast(**kw) == INVALID and "tgs_mesh_rasterize" in msg(), (kw, msg())

    def interp(V=8, F=10, C=3, attr=some, tri=some, n=64, rast=some, out=some):
        return lib.tgs_mesh_interpolate(None, V, F, C, attr, tri, n, rast, out)
    for kw in (dict(V=-1), dict(F=-1), dict(C=0), dict(C=-2), dict(n=-1), dict(attr=None), dict(tri=None), dict(rast=None), dict(out=None), dict(n=1 << 62, C=4)):
        assert interp(**kw) == INVALID and "tgs_mesh_interpolate" in msg(), (kw, msg())
    assert interp(n=0) == 0                                        # no pixels: nothing is launched


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_raster as dr
    assert isinstance(dr.RasterizeCudaContext(device="cuda"), dr.RasterizeCudaContext)
    assert not hasattr(dr, "antialias")                            # not an identity under that name: INTEGRATION.md 4j gives the edit instead
    pos, tri = torch.zeros(1, 3, 4), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rast, attr = torch.zeros(1, 4, 4, 4), torch.zeros(3, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):         # CPU tensors, like knn.py
        dr.rasterize(None, pos, tri, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dr.interpolate(attr, rast, tri)
    # wrong dtype or shape
    for bad_pos in (pos.double(), torch.zeros(3, 3), torch.zeros(1, 1, 3, 4)):
        with pytest.raises(RuntimeError, match="pos"):
            dr.rasterize(None, bad_pos, tri, (4, 4))
    for bad_tri in (tri.long(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="tri"):
            dr.rasterize(None, pos, bad_tri, (4, 4))
        with pytest.raises(RuntimeError, match="tri"):
            dr.interpolate(attr, rast, bad_tri)
    for bad_res in ((0, 4), (4, 8193), (4,)):
        with pytest.raises(RuntimeError, match="resolution"):
            dr.rasterize(None, pos, tri, bad_res)
    for bad_rast in (rast.double(), torch.zeros(4, 4, 4), torch.zeros(1, 4, 4, 3)):
        with pytest.raises(RuntimeError, match="rast"):
            dr.interpolate(attr, bad_rast, tri)
    for bad_attr in (attr.half(), torch.zeros(3), torch.zeros(2, 3, 2), torch.zeros(3, 0)):
        with pytest.raises(RuntimeError, match="attr"):
            dr.interpolate(bad_attr, rast, tri)
    # forward only: an input that requires a gradient is refused, not detached
    with pytest.raises(RuntimeError, match="forward only"):
        dr.rasterize(None, pos.clone().requires_grad_(True), tri, (4, 4))
    with pytest.raises(RuntimeError, match="forward only"):
        dr.interpolate(attr.clone().requires_grad_(True), rast, tri)
    with pytest.raises(RuntimeError, match="forward only"):
        dr.interpolate(attr, rast.clone().requires_grad_(True), tri)
    # an index outside [0, V) raises ValueError before anything is launched
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="vertex indices"):
            dr.rasterize(None, pos, torch.tensor(bad, dtype=torch.int32), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):         # validate=False leaves it to the kernels, which read nothing through it
        dr.rasterize(None, pos, torch.tensor([[0, 1, 3]], dtype=torch.int32), (4, 4), validate=False)
    # more faces than a float carries IDs for (an expanded view: no memory behind it)
    too_many = torch.zeros(1, 3, dtype=torch.int32).expand(1 << 24, 3)
    with pytest.raises(RuntimeError, match="2\\^24"):
        dr.rasterize(None, pos, too_many, (4, 4))
    with pytest.raises(RuntimeError, match="2\\^24"):
        dr.interpolate(attr, rast, too_many)


def test_face_ids_and_hit_faces_on_the_host():
    """they are torch on top of rast: the arithmetic is the same on any device"""
    import youreditableavatar_amd.mesh_raster as dr
    rast = torch.zeros(1, 2, 3, 4)
    rast[0, 0, 1, 3], rast[0, 1, 2, 3], rast[0, 1, 0, 3] = 3.0, 1.0, 16777215.0
    ids = dr.face_ids(rast)
    assert ids.dtype == torch.int32 and ids.tolist() == [[[-1, 2, -1], [16777214, -1, 0]]]
    mask = torch.tensor([[1, 1, 0], [0, 0, 1]])
    assert dr.hit_faces(rast, mask, num_faces=4).tolist() == [True, False, True, False]
    assert dr.hit_faces(rast[0], mask != 0, num_faces=3).tolist() == [True, False, True]
    with pytest.raises(RuntimeError):
        dr.hit_faces(rast, torch.zeros(3, 2))


def test_the_docs_say_what_changes_without_antialias():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4j" in text or "### 4j" in text
    sec = text[text.index("4j"):]
    for what in ("mesh_raster", "dr.antialias", "mask_mesh", "prepare_mask_proj", "get_concat_mask", "gb_normal_aa", "one-pixel", "no clipping", "hit_faces"):
        assert what in sec, what
    survey = open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "4j" in survey
