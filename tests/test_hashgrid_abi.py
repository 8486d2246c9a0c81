"""CPU: the hash-grid field at the C ABI and in youreditableavatar_amd.hashgrid (no device needed): the header declares and the cross-compiled library
exports the entry points, the header states the rules, the signature table matches the header, the workspace size is what the design needs, bad
arguments are refused before any device call, the module refuses what it cannot serve, with messages, and the mesh rasterizer's gradients build from
the shared fixed-point header."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import hashgrid_ref as R
from tests.util import ROOT

HEADER = os.path.join(ROOT, "include", "tgs_raster.h")
CSRC = os.path.join(ROOT, "youreditableavatar_amd", "csrc")
NEW = ("tgs_hashgrid_workspace_bytes", "tgs_hashgrid_encode", "tgs_hashgrid_encode_backward", "tgs_hashgrid_field", "tgs_hashgrid_field_backward")
INVALID = -1
SLABS = 1024 * (64 * 32 + 4 * 64) * 8                                            # the fused backward's partial sums, in bytes


def lib_path():
    from youreditableavatar_amd import build
    return build.build_native()


def _lib():
    from youreditableavatar_amd import hashgrid
    lib = hashgrid.declare(ctypes.CDLL(lib_path()))          # its own handle, the module's signature table
    lib.tgs_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tgs_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    assert re.search(r"size_t\s+tgs_hashgrid_workspace_bytes\(int64_t n_params, int hidden, int n_out\);", src)
    assert src.index("tgs_meshgeom_laplacian_backward(") < src.index("tgs_hashgrid_workspace_bytes(")
    assert text.index("---- mesh geometry ----") < text.index("---- hash-grid field ----")
    block = text[text.index("---- hash-grid field ----"):]
    block = block[:block.index("tgs_hashgrid_field_backward(")]
    for rule in ("computed ONCE, on the host", "never recomputed on the device", "exp2(l * log2(per_level_scale)) * base_resolution - 1", "ceil(scale) + 1",
                 "min(round_up(resolution^3, 8), 2^log2_hashmap_size)", "running sum", "dense = resolution^3 <= size", "at most 16 records", "no device allocation", "no\n * read-back",
                 "params[(offset + index) * 2 + f]", "published layout of tiny-cuda-nn", "has not been compared against tiny-cuda-nn", "pos = x * scale + 0.5", "floor(pos)",
                 "evaluated in double", "product\n *                is exact", "taken as uint32", "cx + cy * res + cz * res^2", "cx * 1 ^ cy * 2654435761 ^ cz * 805459861",
                 "ALWAYS taken % size", "aliases into the next row", "rounded to fp32 once", "exact zeros", "ProgressiveBandHashGrid", "non-finite coordinate", "row of NaN",
                 "contributes nothing", "first-order derivative", "no scatter", "(x - bbox_min) / (bbox_max - bbox_min)", "relu(W1 enc)", "W2 h + bias", "{16, 32, 64}",
                 "1 <= n_out <= 4", "Nothing of size N x 2 n_levels or N x hidden", "recomputes enc and h", "no dL_dx on the fused path", "no float atomics",
                 "never read back", "max |dL_denc|", "ANALYTIC upper bound", "max_j sum_k sum_o |W1[k,j]| |W2[o,k]|", "llrint(c 2^(34 - e))", "2^28 contributions",
                 "one no-return 64-bit integer atomic", "one rounding", "Elements that no point reaches are exact zeros", "non-finite bound makes that gradient all NaN",
                 "per-workgroup partial", "ascending workgroup order", "Two runs give the same bits", "stored, not accumulated", "TGS_ERR_INVALID", "before any device call",
                 "n_input_dims == 3", "n_features == 2", "1 <= n_levels <= 16", "3 <= log2_hashmap_size <= 24", "0 <= N <= 2^25", "8 bytes per parameter", "allocate nothing"):
        assert rule in block, rule
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    from youreditableavatar_amd import build, hashgrid
    assert "tgs_hashgrid.hip" in build.SOURCES
    assert set(hashgrid.SIGNATURES) == set(NEW)
    for name, (_, argtypes) in hashgrid.SIGNATURES.items():                 # the table has as many arguments as the header's declaration
        decl = re.search(name + r"\(([^;]*)\);", src).group(1)
        assert len(argtypes) == len(decl.split(",")), name
        for ctype, arg in zip(argtypes, decl.split(",")):                    # and the same kinds: pointers, int, int64_t, size_t, float
            want = ctypes.c_void_p if "*" in arg else ctypes.c_int64 if "int64_t" in arg else ctypes.c_size_t if "size_t" in arg else ctypes.c_float if "float" in arg else ctypes.c_int
            assert ctype is want, (name, arg)
    fields = re.search(r"typedef struct \{([^}]*)\} tgs_hashgrid_level_t;", src).group(1)
    assert [f.split()[-1] for f in fields.split(";") if f.strip()] == [n for n, _ in hashgrid._LevelRec._fields_]
    assert ctypes.sizeof(hashgrid._LevelRec) == 20


def test_workspace_size():
    ws = _lib().tgs_hashgrid_workspace_bytes
    n = 12196240                                                             # the default config
    assert 8 * n <= ws(n, 0, 0) <= 8 * n + 4096                              # 8 bytes per accumulated element, a small constant
    for H, D in ((16, 1), (32, 4), (64, 1), (64, 4)):
        assert 8 * n + SLABS <= ws(n, H, D) <= 8 * n + SLABS + 4096          # plus the partial slabs
    assert 8 * 16 <= ws(16, 0, 0) <= 8 * 16 + 4096
    for bad in ((0, 0, 0), (-1, 0, 0), (15, 0, 0), (2 * 16 * (1 << 24) + 2, 0, 0), (n, 8, 1), (n, 128, 1), (n, 64, 0), (n, 64, 5), (n, 48, 1)):
        assert ws(*bad) == 0, bad


def _table(name="odd"):
    from youreditableavatar_amd import hashgrid
    levels = hashgrid.level_table(R.CONFIGS[name])
    return hashgrid._records(levels), len(levels), R.CONFIGS[name]["log2_hashmap_size"], 2 * R.n_entries(levels)


def test_invalid_arguments_are_rejected_before_any_device_call():
    from youreditableavatar_amd import hashgrid
    lib = _lib()
    some, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)     # never dereferenced: every call below must fail in the argument checks
    msg = lambda: (lib.tgs_last_error() or b"").decode()
    recs, L, log2, n_params = _table()
    big, fbig = lib.tgs_hashgrid_workspace_bytes(n_params, 0, 0), lib.tgs_hashgrid_workspace_bytes(n_params, 32, 4)
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)

    def broken(**kw):                                              # the table with one field of one record changed
        out = hashgrid._records(hashgrid.level_table(R.CONFIGS["odd"]))
        for k, v in kw.items():
            setattr(out[2], k, v)
        return out
    head = dict(N=100, dims=3, x=some, params=some, levels=recs, n_levels=L, feats=2, log2=log2, active=L)
    bad_heads = [dict(N=-1), dict(N=(1 << 25) + 1), dict(dims=2), dict(dims=4), dict(x=None), dict(params=None), dict(levels=None), dict(n_levels=0), dict(n_levels=17), dict(feats=1),
                 dict(feats=4), dict(log2=2), dict(log2=25), dict(log2=7), dict(active=-1), dict(active=L + 1), dict(levels=broken(offset=1)), dict(levels=broken(size=257)),
                 dict(levels=broken(size=512)), dict(levels=broken(dense=1)), dict(levels=broken(dense=2)), dict(levels=broken(scale=float("nan"))), dict(levels=broken(scale=-1.0)),
                 dict(levels=broken(scale=2.0 ** 20)), dict(levels=broken(resolution=0))]

    def call(fn, tail, **kw):
        a = dict(head, **{k: v for k, v in kw.items() if k in head})
        t = dict(tail, **{k: v for k, v in kw.items() if k not in head})
        return fn(None, a["N"], a["dims"], a["x"], a["params"], a["levels"], a["n_levels"], a["feats"], a["log2"], a["active"], *t.values())

    mlp = dict(bbox=box, W1=some, W2=some, hidden=32, n_out=4)
    bad_mlps = [dict(W1=None), dict(W2=None), dict(hidden=0), dict(hidden=8), dict(hidden=48), dict(hidden=128), dict(n_out=0), dict(n_out=5),
                dict(bbox=(ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)), dict(bbox=(ctypes.c_float * 6)(0, 0, 0, 1, float("nan"), 1)), dict(bbox=(ctypes.c_float * 6)(0, 0, 0, 1, float("inf"), 1))]
    tails = {
        "tgs_hashgrid_encode": (dict(enc=other), [dict(enc=None)]),
        "tgs_hashgrid_encode_backward": (dict(g=some, d_params=other, d_x=other, ws=some, nbytes=big), [dict(g=None), dict(ws=None), dict(nbytes=big - 1), dict(nbytes=0)]),
        "tgs_hashgrid_field": (dict(mlp, bias=0.5, out=other), bad_mlps + [dict(out=None)]),
        "tgs_hashgrid_field_backward": (dict(mlp, g=some, d_params=other, d_W1=other, d_W2=other, ws=some, nbytes=fbig),
                                        bad_mlps + [dict(g=None), dict(ws=None), dict(nbytes=fbig - 1), dict(nbytes=big), dict(nbytes=0)]),
    }
    for name, (tail, bad_tails) in tails.items():
        for kw in bad_heads + bad_tails:
            assert call(getattr(lib, name), tail, **kw) == INVALID and name + ":" in msg(), (name, kw, msg())
    call(lib.tgs_hashgrid_encode, tails["tgs_hashgrid_encode"][0], N=(1 << 25) + 1)
    assert "2^25" in msg() and "chunks" in msg()
    # nothing to do: no device call either
    assert call(lib.tgs_hashgrid_encode, tails["tgs_hashgrid_encode"][0], N=0, x=None, enc=None) == 0
    assert call(lib.tgs_hashgrid_field, tails["tgs_hashgrid_field"][0], N=0, x=None, out=None) == 0
    assert call(lib.tgs_hashgrid_field_backward, tails["tgs_hashgrid_field_backward"][0], d_params=None, d_W1=None, d_W2=None) == 0


def test_the_module_refuses_what_it_cannot_serve():
    import youreditableavatar_amd.hashgrid as hg
    for what in ("no CPU path", "tiny-cuda-nn", "nobody could check", 'normal_type="analytic"', "n_feature_dims > 0", "isosurface_chunk", "no float atomics"):
        assert what in hg.__doc__, what
    cfg = R.CONFIGS["odd"]
    with pytest.raises(RuntimeError, match="3 input dimensions"):
        hg.HashGrid(2, cfg)
    with pytest.raises(RuntimeError, match="no half precision"):
        hg.HashGrid(3, cfg, dtype=torch.float16)
    for bad, why in ((dict(cfg, n_features_per_level=4), "2 features per level"), (dict(cfg, interpolation="Smoothstep"), "'Linear' is"), (dict(cfg, type="Dense"), "dense and tiled grids"),
                     (dict(cfg, type="Tiled"), "dense and tiled grids"), (dict(cfg, otype="Frequency"), "is not served"), (dict(cfg, otype="DenseGrid"), "is not served"),
                     (dict(cfg, n_levels=17), r"n_levels must be an int in \[1, 16\]"), (dict(cfg, n_levels=0), "n_levels must be"), (dict(cfg, log2_hashmap_size=25), r"in \[3, 24\]"),
                     (dict(cfg, per_level_scale=0.5), "must be >= 1"), (dict(cfg, colour="red"), "unknown keys"), (7, "must be a mapping")):
        with pytest.raises(RuntimeError, match=why):
            hg.HashGrid(3, bad)
        with pytest.raises(RuntimeError, match=why):
            hg.level_table(bad)
    grid = hg.HashGrid(3, dict(cfg, otype="ProgressiveBandHashGrid", start_level=2, start_step=0, update_steps=100))      # the schedule keys are ignored
    assert grid.n_input_dims == 3 and grid.n_output_dims == 10 and grid.params.numel() == 2 * (32 + 128 + 3 * 256) and isinstance(grid.params, torch.nn.Parameter)
    assert 0 < float(grid.params.detach().abs().max()) <= 1e-4
    levels = list(grid.levels)
    shifted = [levels[0]] + [v._replace(offset=v.offset + 8) for v in levels[1:]]
    with pytest.raises(RuntimeError, match="level 1 of the table is inconsistent"):
        hg.HashGrid(3, cfg, levels=shifted)
    with pytest.raises(RuntimeError, match="levels has 4 records"):
        hg.HashGrid(3, cfg, levels=levels[:4])
    explicit = hg.HashGrid(3, cfg, levels=[levels[0]._replace(scale=2.25)] + levels[1:])        # a producer that rounded a scale otherwise
    assert explicit.levels[0].scale == 2.25 and explicit.params.numel() == grid.params.numel()

    x, P = torch.zeros(5, 3), grid.params.detach()
    W1, W2 = torch.zeros(32, 10), torch.zeros(4, 32)
    with pytest.raises(RuntimeError, match="x must be a tensor"):
        hg.hashgrid_encode([[0, 0, 0]], P, levels)
    for bad in (x.double(), x[:, :2], x[0]):
        with pytest.raises(RuntimeError, match=r"float32 x of shape \[N,3\]"):
            hg.hashgrid_encode(bad, P, levels)
        with pytest.raises(RuntimeError, match=r"float32 x of shape \[N,3\]"):
            hg.sdf_field(bad, P, levels, W1, W2)
    with pytest.raises(RuntimeError, match="isosurface_chunk"):
        hg.hashgrid_encode(torch.zeros(1, 3).expand((1 << 25) + 1, 3), P, levels)                 # (a view of one row: no memory)
    with pytest.raises(RuntimeError, match="isosurface_chunk"):
        grid(torch.zeros(1, 3).expand((1 << 25) + 1, 3))
    with pytest.raises(RuntimeError, match=r"float32 params of shape \[1856\]"):
        hg.hashgrid_encode(x, P[:-2], levels)
    with pytest.raises(RuntimeError, match=r"float32 params of shape"):
        hg.hashgrid_encode(x, P.double(), levels)
    with pytest.raises(RuntimeError, match="list of 1 to 16 Level records"):
        hg.hashgrid_encode(x, P, [(1.0, 2, 8, 0, True)])
    for bad in (-1, 6, 2.0, True):
        with pytest.raises(RuntimeError, match="active_levels must be None or an int"):
            hg.hashgrid_encode(x, P, levels, bad)
    for a, b in ((torch.zeros(32, 8), W2), (W1, torch.zeros(4, 16)), (W1.double(), W2), (W1[0], W2)):
        with pytest.raises(RuntimeError, match="W1|W2"):
            hg.sdf_field(x, P, levels, a, b)
    with pytest.raises(RuntimeError, match="hidden width of 16, 32 or 64 and 1 to 4 outputs"):
        hg.sdf_field(x, P, levels, torch.zeros(48, 10), torch.zeros(1, 48))
    with pytest.raises(RuntimeError, match="hidden width of 16, 32 or 64 and 1 to 4 outputs"):
        hg.sdf_field(x, P, levels, W1, torch.zeros(5, 32))
    for bad in ([[0, 0, 0], [1, 0, 1]], [[0, 0, 0]], [[0, 0, 0], [1, float("inf"), 1]]):
        with pytest.raises(RuntimeError, match="bbox must be"):
            hg.sdf_field(x, P, levels, W1, W2, bbox=bad)
    with pytest.raises(RuntimeError, match="encoding must be a HashGrid"):
        hg.SdfField(torch.nn.Identity(), W1, W2)
    # which networks the fused kernel covers
    lin = lambda i, o, bias=False: torch.nn.Linear(i, o, bias=bias)
    seq = torch.nn.Sequential
    assert hg.SdfField(grid, W1, W2).fused and hg.SdfField(grid, seq(lin(10, 64), torch.nn.ReLU(inplace=True), lin(64, 1))).fused
    for net in (seq(lin(10, 64), torch.nn.ReLU(), lin(64, 64), torch.nn.ReLU(), lin(64, 1)), seq(lin(10, 48), torch.nn.ReLU(), lin(48, 1)),
                seq(lin(10, 64, True), torch.nn.ReLU(), lin(64, 1)), seq(lin(10, 64), torch.nn.Softplus(), lin(64, 1)), seq(lin(10, 64), torch.nn.ReLU(), lin(64, 5))):
        assert not hg.SdfField(grid, net).fused
    # the device check comes last
    for p in (x, x.clone().requires_grad_(True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            hg.hashgrid_encode(p, P, levels)
        with pytest.raises(RuntimeError, match="no CPU path"):
            grid(p, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hg.sdf_field(x, P, levels, W1, W2, bbox=[[0, 0, 0], [1, 1, 1]], bias=0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hg.SdfField(grid, W1, W2)(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hg.SdfField(grid, seq(lin(10, 48), torch.nn.ReLU(), lin(48, 1)))(x)


def test_the_mesh_gradients_build_from_the_shared_header():
    shared = open(os.path.join(CSRC, "tgs_grad_fixed.hpp")).read()
    for name in ("grad_scale", "grad_fixed", "grad_bound_max", "wave_runs", "run_sum", "k_grad_max_abs", "k_grad_convert", "GRAD_FRAC = 34"):
        assert name in shared, name
    for source in ("tgs_mesh_grad.hip", "tgs_hashgrid.hip"):
        text = open(os.path.join(CSRC, source)).read()
        assert '#include "tgs_grad_fixed.hpp"' in text, source
        for once in ("GRAD_FRAC =", "void k_grad_convert", "void k_grad_max_abs", "bool grad_scale(", "WaveRuns wave_runs("):      # no second copy
            assert once not in text, (source, once)
    syms = subprocess.run(["nm", "-D", lib_path()], capture_output=True, text=True).stdout
    for name in ("tgs_mesh_interpolate_backward", "tgs_mesh_rasterize_backward", "tgs_mesh_antialias_backward", "tgs_hashgrid_field_backward"):
        assert re.search(r" T " + name + r"\b", syms), name


def test_the_docs_have_the_hash_grid_section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 4o" in text and text.index("## 4n") < text.index("## 4o") < text.index("## 5. ")
    sec = text[text.index("## 4o"):text.index("## 5. ")]
    for what in ("from youreditableavatar_amd.hashgrid import", "HashGrid", "SdfField", "hashgrid_encode", "TCNNEncoding", "ProgressiveBandHashGrid", "forward_sdf", "forward_field",
                 "analytic", "n_feature_dims", "tiny-cuda-nn", "isosurface_chunk", "tools/hashgrid_loop.py", "examples/fit_hashgrid_sdf.py"):
        assert what in sec, what
    assert "easured" in sec                                                  # "Measured ..." or "unmeasured"
    assert "hashgrid" in open(os.path.join(ROOT, "README.md")).read()
    assert "hashgrid" in open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "hashgrid" in open(os.path.join(ROOT, "DESIGN.md")).read()
