"""CPU: the mesh rasterizer's gradients at the C ABI and in youreditableavatar_amd.mesh_raster_grad (no device needed): the header declares and
the cross-compiled library exports the four entry points, the header states the rules, bad arguments are refused before any device call, and
the module refuses what it cannot serve while the two older modules stay forward only."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_mesh_grad_workspace_bytes", "tgs_mesh_interpolate_backward", "tgs_mesh_rasterize_backward", "tgs_mesh_antialias_backward")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import _mesh
    lib = _mesh.declare(ctypes.CDLL(lib_path()))            # its own handle, the package's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_gradient_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_mesh_grad_workspace_bytes\(int V, int C, int64_t n_pixels\);", src)
    # a new block behind the antialias block, and the rules' key phrases
    assert src.index("tgs_mesh_antialias(") < src.index("tgs_mesh_grad_workspace_bytes(")
    assert text.index("mesh rasterizer: antialias") < text.index("mesh rasterizer: gradients")
    block = text[text.index("mesh rasterizer: gradients"):]
    block = block[:block.index("tgs_mesh_antialias_backward(")]
    for rule in ("vertex 0's row of dL_dattr[V,C] receives u g", "vertex 1's v g, vertex 2's (1 - u - v) g", "sum_c g_c (a0_c - a2_c)", "sum_c g_c (a1_c - a2_c)",
                 "channels 2 and 3 exact zeros", "q_k = b_k / w_k", "max(u + v, 1)", "1 inside and at the bounds, 0 outside", "The z column", "unsnapped pos",
                 "coverage is not decided again", "is a gather", "left, right, below, above", "One writer per element, no atomics", "is held fixed",
                 "t~ = E(P) / (-D)", "X = (x/w 0.5 + 0.5) width 256", "derivative of snapping is taken as 1", "exit edge's two", "color[O,c] - color[R,c]",
                 "pos_gradient_boost", "contributes nothing backward", "stored, not accumulated", "no float atomics on gradient memory",
                 "integer atomicMax on the float's bits", "llrint(c 2^(34 - e))", "cannot overflow 63 bits", "runs of equal destination", "no-return 64-bit integer atomic",
                 "two runs give the same bits", "n 2^(e-35)", "every element of that gradient is NaN", "dL_dcolor is a copy of dL_dout"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build
    assert "tgs_mesh_grad.hip" in build.SOURCES


def test_workspace_sizes():
    ws = _lib().tgs_mesh_grad_workspace_bytes
    assert ws(0, 1, 0) > 0
    assert ws(1000, 3, 256 * 256) >= 1000 * 4 * 8 + 256 * 256 * 8             # [V,4] 64-bit sums at least, and the two pair records per pixel
    assert ws(1000, 7, 256 * 256) >= 1000 * 7 * 8 + 256 * 256 * 8
    assert ws(1000, 7, 256 * 256) <= 1000 * 7 * 8 + 256 * 256 * 8 + 4096
    assert ws(1000, 3, 512 * 512) > ws(1000, 3, 256 * 256) and ws(2000, 3, 4096) > ws(1000, 3, 4096)
    assert ws(10, 1, 8192 * 8192) > 0
    for bad in ((-1, 3, 16), (8, 0, 16), (8, -2, 16), (8, 3, -1), (8, 3, 8192 * 8192 + 1)):
        assert ws(*bad) == 0, bad


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    big = lib.tgs_mesh_grad_workspace_bytes(8, 4, 64 * 48)

    def interp(V=8, F=10, C=3, attr=some, tri=some, n=64 * 48, rast=some, g=some, d_attr=some, d_rast=other, ws=some, nbytes=big):
        return lib.tgs_mesh_interpolate_backward(None, V, F, C, attr, tri, n, rast, g, d_attr, d_rast, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(C=0), dict(C=-2), dict(n=-1), dict(n=8192 * 8192 + 1), dict(attr=None), dict(tri=None), dict(rast=None),
               dict(g=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0), dict(C=5)):
        assert interp(**kw) == INVALID and "tgs_mesh_interpolate_backward" in msg(), (kw, msg())

    def rast(V=8, F=10, pos=some, tri=some, W=64, H=48, rast=some, g=some, d_pos=other, ws=some, nbytes=big):
        return lib.tgs_mesh_rasterize_backward(None, V, F, pos, tri, W, H, rast, g, d_pos, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(W=0), dict(H=-3), dict(W=8193), dict(H=8193), dict(pos=None), dict(tri=None), dict(rast=None), dict(g=None),
               dict(d_pos=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0)):
        assert rast(**kw) == INVALID and "tgs_mesh_rasterize_backward" in msg(), (kw, msg())
    assert rast(V=0, pos=None, d_pos=None) == 0                   # no vertices: nothing to write, nothing launched

    def aa(V=8, F=10, C=3, pos=some, tri=some, topo=some, W=64, H=48, rast=some, color=some, g=some, d_color=other, d_pos=other, boost=1.0, ws=some, nbytes=big):
        return lib.tgs_mesh_antialias_backward(None, V, F, C, pos, tri, topo, W, H, rast, color, g, d_color, d_pos, boost, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(C=0), dict(C=-2), dict(W=0), dict(H=-3), dict(W=8193), dict(H=8193), dict(pos=None), dict(tri=None),
               dict(topo=None), dict(rast=None), dict(color=None), dict(g=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0), dict(C=5), dict(d_color=some)):
        assert aa(**kw) == INVALID and "tgs_mesh_antialias_backward" in msg(), (kw, msg())
    assert aa(d_color=some) == INVALID and "alias" in msg()
    assert aa(d_color=None, d_pos=None) == 0                      # no gradient wanted: nothing launched


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.mesh_raster as base
    import youreditableavatar_amd.mesh_raster_aa as aa
    import youreditableavatar_amd.mesh_raster_grad as dr
    for name in ("RasterizeCudaContext", "face_ids", "hit_faces"):
        assert getattr(dr, name) is getattr(base, name), name     # re-exported unchanged
    assert dr.antialias_construct_topology_hash is aa.antialias_construct_topology_hash
    assert issubclass(dr.RasterizeGLContext, dr.RasterizeCudaContext) and dr.RasterizeGLContext(device="cuda").device == "cuda"
    for fn in (dr.rasterize, dr.interpolate, dr.antialias):
        assert fn.__module__ == dr.__name__
    assert "ignored" in dr.rasterize.__doc__ and "None" in dr.rasterize.__doc__ and "z/w" in dr.rasterize.__doc__
    pos, tri = torch.zeros(1, 3, 4), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rast, color, attr = torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 2), torch.zeros(3, 2)
    grad = lambda t: t.clone().requires_grad_(True)
    for p in (pos, grad(pos)):                                    # with and without a gradient: the existing checks and messages
        with pytest.raises(RuntimeError, match="no CPU path"):
            dr.rasterize(dr.RasterizeGLContext(), p, tri, (4, 4), grad_db=True)
        with pytest.raises(RuntimeError, match="no CPU path"):
            dr.antialias(color, rast, p, tri, pos_gradient_boost=2.0)
        with pytest.raises(RuntimeError, match="resolution"):
            dr.rasterize(None, p, tri, (4, 0))
    for a, r in ((attr, rast), (grad(attr), rast), (attr, grad(rast))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            dr.interpolate(a, r, tri)
        with pytest.raises(RuntimeError, match="attr"):
            dr.interpolate(a.double(), r, tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dr.antialias(grad(color), rast, pos, tri)
    with pytest.raises(RuntimeError, match="topology"):          # shape and dtype come first, as in mesh_raster_aa
        dr.antialias(grad(color), rast, pos, tri, topology_hash=torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="tri"):
        dr.antialias(grad(color), rast, grad(pos), tri.long())
    # no attribute derivatives
    for kw in (dict(rast_db=rast), dict(diff_attrs="all"), dict(rast_db=rast, diff_attrs=[0])):
        with pytest.raises(RuntimeError, match="rast_db and diff_attrs must be None"):
            dr.interpolate(attr, rast, tri, **kw)
    # the two older modules stay forward only, with their messages
    with pytest.raises(RuntimeError, match="mesh_raster is forward only: `pos` requires a gradient"):
        base.rasterize(None, grad(pos), tri, (4, 4))
    with pytest.raises(RuntimeError, match="mesh_raster is forward only: `attr` requires a gradient"):
        aa.interpolate(grad(attr), rast, tri)
    with pytest.raises(RuntimeError, match="mesh_raster is forward only: `color` requires a gradient"):
        aa.antialias(grad(color), rast, pos, tri)
    for mod in (base, aa):
        assert "mesh_raster_grad" in mod.__doc__


def test_the_docs_have_the_gradient_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4l" in text and text.index("## 4k") < text.index("## 4l") < text.index("## 5. ")
    sec = text[text.index("## 4l"):text.index("## 5. ")]
    for what in ("import youreditableavatar_amd.mesh_raster_grad as dr", "rast_db", "z/w", "snapped", "4k", "pos_gradient_boost", "fixed point", "tools/mesh_grad_loop.py",
                 "examples/fit_mesh_silhouette_normals.py", "Measured"):
        assert what in sec, what
    assert "mesh_raster_grad" in open(os.path.join(ROOT, "README.md")).read()
