"""CPU: mesh shading at the C ABI and in youreditableavatar_amd.mesh_shade (no device needed): the header declares and the cross-compiled
library exports the three entry points, the header states the rules, the signature table agrees with the header, bad arguments are refused
before any device call, and the module checks its arguments in the siblings' order: types and shapes, then tri, then the device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
NEW = ("tgs_meshshade_workspace_bytes", "tgs_meshshade", "tgs_meshshade_backward")
INVALID = -1


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import _mesh
    lib = _mesh.declare(ctypes.CDLL(lib_path()))            # its own handle, the package's signature tables
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_meshshade_workspace_bytes\(int V, int C, int64_t n_pixels\);", src)
    assert text.index("mesh rasterizer: gradients") < text.index("---- mesh shading ----") < text.index("---- marching tetrahedra ----")
    block = text[text.index("---- mesh shading ----"):]
    block = block[:block.index("tgs_meshshade_backward(")]
    for rule in ("m = u a0 + v a1 + (1 - u - v) a2", "Channel 0 is 1", "n = m / max(|m|, 1e-12)", "(n.y, n.z, n.x)", "m' = R^-1 m", "adjugate over determinant",
                 "if flip", "m'.z < 0", "(n + 1) / 2", "d = 1 / (z + 1e-7)", "(d - dmin) / (dmax - dmin + 1e-7)", "order-preserving", "does not depend on the order of arrival",
                 "never read back", "exact zeros in every channel", "Two departures", "normals NaN", "all-zero depth channel", "Channel 0 of g is ignored",
                 "g_n = g / 2", "(g_n - n (n . g_n)) / |m'|", "g_n / 1e-12", "R^-T", "r = dmax - dmin + 1e-7", "-S2 / r^2", "-S1 / r + S2 / r^2", "S1 = sum g_q",
                 "ascending workgroup order", "dL/dz = -dL/dd d^2", "sum_c g_c (a0_c - a2_c)", "channels 2 and 3 exact zeros", "one shared header", "llrint(c 2^(34 - e))",
                 "runs of equal destination", "no-return 64-bit integer atomic", "no float atomics", "two runs give the same bits", "every element of that gradient tensor NaN"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build
    assert "tgs_mesh_shade.hip" in build.SOURCES
    kernel = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_shade.hip")).read()
    grad = open(os.path.join(ROOT, "youreditableavatar_amd", "csrc", "tgs_mesh_grad.hip")).read()
    assert '#include "tgs_grad_fixed.hpp"' in kernel and '#include "tgs_grad_fixed.hpp"' in grad      # the scatter's machinery: one header, no copy
    for name in ("grad_fixed(", "wave_runs(", "run_sum(", "grad_add(", "k_grad_convert"):
        assert name in kernel and not re.search(r"(void|long long|WaveRuns|bool)\s+" + re.escape(name), kernel), name
    assert "atomicAdd(float" not in kernel and "asm" not in kernel


def test_the_signature_table_agrees_with_the_header():
    from youreditableavatar_amd import _mesh
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}

    def kind(decl):
        decl = decl.strip()
        return ctypes.c_void_p if "*" in decl else kinds[[w for w in decl.split() if w != "const"][0]]
    protos = re.findall(r"([A-Za-z_0-9]+[\s\*]+)(tgs_meshshade[a-z0-9_]*)\s*\(([^)]*)\)\s*;", src)
    declared = {name: (kind(ret), [kind(p) for p in params.split(",")]) for ret, name, params in protos}
    assert len(protos) == len(declared) == 3 and set(_mesh.SHADE_SIGNATURES) == set(declared) == set(NEW)
    for name, (restype, argtypes) in declared.items():
        assert _mesh.SHADE_SIGNATURES[name][0] is restype and list(_mesh.SHADE_SIGNATURES[name][1]) == argtypes, name
    assert not set(_mesh.SHADE_SIGNATURES) & set(_mesh.SIGNATURES)


def test_workspace_sizes():
    ws = _lib().tgs_meshshade_workspace_bytes
    assert ws(0, 4, 0) > 0 and ws(0, 5, 0) > 0
    groups = lambda n: (n + 255) // 256
    for V, n in ((1000, 256 * 256), (12, 7 * 5), (70000, 1024 * 1024)):
        need = V * 4 * 8 + groups(n) * 4 * 8                                     # [V,3] + [V] 64-bit sums, four doubles per workgroup of 256 pixels
        assert need <= ws(V, 5, n) <= need + 4096, (V, n, ws(V, 5, n), need)
        assert ws(V, 4, n) == ws(V, 5, n)
    assert ws(1000, 5, 512 * 512) > ws(1000, 5, 256 * 256) and ws(2000, 5, 4096) > ws(1000, 5, 4096)
    assert ws(10, 4, 8192 * 8192) > 0
    for bad in ((-1, 4, 16), (8, 3, 16), (8, 6, 16), (8, 0, 16), (8, 4, -1), (8, 5, 8192 * 8192 + 1)):
        assert ws(*bad) == 0, bad


def test_invalid_arguments_are_rejected_before_any_device_call():
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    big = lib.tgs_meshshade_workspace_bytes(8, 5, 64 * 48)

    def fwd(V=8, F=10, tri=some, vn=some, z=some, camera=1, rot=some, flip=1, n=64 * 48, rast=some, out=other, ws=some, nbytes=big):
        return lib.tgs_meshshade(None, V, F, tri, vn, z, camera, rot, flip, n, rast, out, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(n=-1), dict(n=8192 * 8192 + 1), dict(tri=None), dict(vn=None), dict(rot=None), dict(camera=2), dict(camera=-1),
               dict(flip=2), dict(rast=None), dict(out=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0)):
        assert fwd(**kw) == INVALID and "tgs_meshshade:" in msg(), (kw, msg())
    assert fwd(n=0, rast=None, out=None) == 0                      # no pixels: nothing to write, nothing launched

    def bwd(V=8, F=10, tri=some, vn=some, z=some, camera=1, rot=some, flip=1, n=64 * 48, rast=some, g=some, d_vn=other, d_z=other, d_rast=other, ws=some, nbytes=big):
        return lib.tgs_meshshade_backward(None, V, F, tri, vn, z, camera, rot, flip, n, rast, g, d_vn, d_z, d_rast, ws, nbytes)
    for kw in (dict(V=-1), dict(F=-1), dict(F=1 << 24), dict(n=-1), dict(n=8192 * 8192 + 1), dict(tri=None), dict(vn=None), dict(rot=None), dict(camera=2), dict(flip=-1),
               dict(rast=None), dict(g=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0), dict(z=None)):
        assert bwd(**kw) == INVALID and "tgs_meshshade_backward:" in msg(), (kw, msg())
    assert bwd(d_vn=None, d_z=None, d_rast=None) == 0              # no gradient wanted: nothing launched
    assert bwd(z=None, d_z=None, d_vn=None, d_rast=None, camera=0, rot=None) == 0


def test_the_module_checks_its_arguments():
    import youreditableavatar_amd.mesh_shade as ms
    for fn in (ms.shade, ms.render):
        assert fn.__module__ == ms.__name__
    for what in ("singular", "no covered pixel", "never receives a gradient"):
        assert what in ms.__doc__ + ms.shade.__doc__, what
    N, H, W, V = 2, 4, 5, 3
    rast, tri, vn = torch.zeros(N, H, W, 4), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros(V, 3)
    c2w, pos = torch.eye(4)[None].repeat(N, 1, 1), torch.zeros(V, 4)
    grad = lambda t: t.clone().requires_grad_(True)
    for r, n in ((rast, vn), (grad(rast), vn), (rast, grad(vn))):                 # with and without a gradient: the same checks and messages
        with pytest.raises(RuntimeError, match="rast and vn must be tensors"):
            ms.shade(None, tri, n, c2w=c2w)
        with pytest.raises(RuntimeError, match=r"expected float32 rast of shape \[N,H,W,4\]"):
            ms.shade(r[0], tri, n, c2w=c2w)
        with pytest.raises(RuntimeError, match="expected float32 vn of shape"):
            ms.shade(r, tri, n.double(), c2w=c2w)
        with pytest.raises(RuntimeError, match="expected float32 vn of shape"):
            ms.shade(r, tri, n[None].repeat(3, 1, 1), c2w=c2w)
        with pytest.raises(ValueError, match="Unknown normal type: view"):
            ms.shade(r, tri, n, normal_type="view", c2w=c2w)
        with pytest.raises(RuntimeError, match="c2w must be None"):
            ms.shade(r, tri, n, normal_type="world", c2w=c2w)
        with pytest.raises(RuntimeError, match="needs c2w"):
            ms.shade(r, tri, n)
        for bad in (c2w.double(), c2w[:, :3], torch.eye(4)[None].repeat(3, 1, 1), torch.eye(2), torch.zeros(())):
            with pytest.raises(RuntimeError, match="expected float32 c2w of shape"):
                ms.shade(r, tri, n, c2w=bad)
        with pytest.raises(RuntimeError, match="flip must be True or False"):
            ms.shade(r, tri, n, c2w=c2w, flip=None)
        with pytest.raises(RuntimeError, match="pos_clip must be a tensor or None"):
            ms.shade(r, tri, n, c2w=c2w, pos_clip=3.0)
        for bad in (pos.double(), torch.zeros(V + 1, 4), torch.zeros(V, 3), torch.zeros(3, V, 4)):
            with pytest.raises(RuntimeError, match="expected float32 pos_clip of shape"):
                ms.shade(r, tri, n, c2w=c2w, pos_clip=bad)
        with pytest.raises(RuntimeError, match="expected int32 tri"):             # tri behind the shapes
            ms.shade(r, tri.long(), n, c2w=c2w)
        with pytest.raises(RuntimeError, match="expected float32 vn"):            # ... and a bad shape in front of a bad tri
            ms.shade(r, tri.long(), n.double(), c2w=c2w)
        for kw in (dict(c2w=c2w), dict(c2w=c2w[0]), dict(c2w=c2w[:1, :3, :3]), dict(normal_type="world"), dict(c2w=c2w, pos_clip=pos), dict(c2w=c2w, flip=False)):
            with pytest.raises(RuntimeError, match="mesh_shade has no CPU path"):  # the device last
                ms.shade(r, tri, n, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ms.render(None, torch.zeros(V, 3), tri, torch.eye(4)[None], (4, 4), c2w=torch.eye(4)[None])
    with pytest.raises(RuntimeError, match="resolution"):
        ms.render(None, torch.zeros(V, 3), tri, torch.eye(4)[None], (4, 0), c2w=torch.eye(4)[None])


def test_the_docs_have_the_shading_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4t" in text and text.index("## 4s") < text.index("## 4t") < text.index("## 5. ")
    sec = text[text.index("## 4t"):text.index("## 5. ")]
    for what in ("youreditableavatar_amd.mesh_shade", "part_nvdiff_rasterizer", "initialize_shape", "flip=False", "singular", "no covered pixel", "c2w", "mvp",
                 "use_additional_input", "tools/mesh_shade_loop.py", "examples/fit_mesh_render.py", "Measured", "launches", "synchronis"):
        assert what in sec, what
    for doc in ("README.md", "SURVEY.md", "DESIGN.md"):
        assert "mesh_shade" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "tools", "mesh_shade_loop.py")) and os.path.exists(os.path.join(ROOT, "examples", "fit_mesh_render.py"))
