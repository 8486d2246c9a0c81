"""CPU: the one host layer under the geometry stage's modules (youreditableavatar_amd/_host.py; no device needed): every module works with _host's own
objects, none keeps a copy of a helper, and each module's ``declare`` sets exactly its own signature table."""
import ctypes
import importlib
import os

import pytest

from tests.util import ROOT

PACKAGE = os.path.join(ROOT, "youreditableavatar_amd")
MODULES = ("_mesh", "marching_tets", "mesh_geom", "hashgrid", "tet_grid")            # with _host itself: the six files of the layer
# module: {its name for the helper: _host's name}
USES = {
    "_mesh": dict(_lib="lib", _raw_stream="raw_stream", _NO_GUARD="NO_GUARD", _need_device="need_device", _ok="ok"),
    "marching_tets": dict(_lib="lib", _ok="ok", _guard="guard", _raw_stream="raw_stream", _workspace="workspace", _index_rows="index_rows", _index_error="index_error"),
    "mesh_geom": dict(_lib="lib", _ok="ok", _guard="guard", _raw_stream="raw_stream", _need_device="need_device", _index_error="index_error"),
    "hashgrid": dict(_lib="lib", _ok="ok", _guard="guard", _raw_stream="raw_stream", _need_device="need_device"),
    "tet_grid": dict(_lib="lib", _ok="ok", _guard="guard", _raw_stream="raw_stream", _workspace="workspace", _rows="index_rows", _ptr="ptr", _index_error="index_error"),
}


def _module(name):
    return importlib.import_module("youreditableavatar_amd." + name)


@pytest.mark.parametrize("name", MODULES)
def test_the_helpers_are_the_host_layers_own(name):
    host, mod = _module("_host"), _module(name)
    for mine, theirs in USES[name].items():
        assert getattr(mod, mine) is getattr(host, theirs), (name, mine)
    for alias in ("_P", "_I", "_L", "_Z", "_F"):
        if hasattr(mod, alias):
            assert getattr(mod, alias) is getattr(host, alias), (name, alias)
    assert host.lib is _module("diff_gaussian_rasterization._C")._lib
    if name != "_mesh":                                                          # the rasterizer's private layer is nobody else's
        text = open(os.path.join(PACKAGE, name + ".py")).read()
        assert "import _mesh" not in text and "_mesh." not in text and "._mesh" not in text, name
    tg, mt = _module("tet_grid"), _module("marching_tets")
    assert tg.check is mt.check and tg.MASK_TYPES is mt.MASK_TYPES and tg.marching_tets is mt.marching_tets     # the kind-based argument check exists once


def test_no_module_keeps_a_copy():
    for name in MODULES:
        text = open(os.path.join(PACKAGE, name + ".py")).read()
        for copy in ("def _ok", "def _guard", "def _need_device", ".restype, getattr(", "contextlib.nullcontext", "_cuda_getCurrentRawStream", "data_ptr() % 16",
                     "holds a vertex index outside", "has no CPU path"):
            assert copy not in text, (name, copy)
    text = open(os.path.join(PACKAGE, "_host.py")).read()
    for once in ("def ok(", "def guard(", "def need_device(", ".restype, getattr(", "contextlib.nullcontext", "_cuda_getCurrentRawStream", "data_ptr() % 16",
                 "holds a vertex index outside", "dtype=torch.uint8", "has no CPU path", "must be on one device"):
        assert text.count(once) == 1, once
    assert text.count("1.9 us of a 17 us call") == 1                             # the comment about the stream's cost moved with it


def test_the_messages_are_word_for_word():
    import torch
    host = _module("_host")
    a, b = torch.zeros(2), torch.zeros(3)
    with pytest.raises(RuntimeError) as e:
        host.need_device("mesh_geom", v_pos=a, faces=b)
    assert str(e.value) == "youreditableavatar_amd.mesh_geom has no CPU path: v_pos must be on a HIP device"

    class OnDevice:                                                              # what need_device reads of a tensor
        def __init__(self, device):
            self.is_cuda, self.device = True, device
    with pytest.raises(RuntimeError) as e:
        host.need_device("hashgrid", x=OnDevice(torch.device("cuda:0")), params=OnDevice(torch.device("cuda:1")))
    assert str(e.value) == "all tensors must be on one device, got x on cuda:0, params on cuda:1"
    assert host.need_device("tet_grid", pos=OnDevice(torch.device("cuda:1")), tet=OnDevice(torch.device("cuda:1"))) == torch.device("cuda:1")
    assert str(host.index_error("tet", 7, "pos has 7 rows")) == "tet holds a vertex index outside [0, 7): pos has 7 rows (code -1)"
    assert str(host.index_error("faces", 0, "the mesh has 0 vertices")) == "faces holds a vertex index outside [0, 0): the mesh has 0 vertices (code -1)"
    assert host.ptr(None) is None and host.ptr(a) == a.data_ptr()
    rows = torch.arange(24, dtype=torch.int32)
    whole, inside = rows[4:20].view(4, 4), rows[1:17].view(4, 4)                 # 16 bytes into the storage, and 4
    assert host.index_rows(whole).data_ptr() == whole.data_ptr()
    moved = host.index_rows(inside)
    assert moved.data_ptr() != inside.data_ptr() and moved.data_ptr() % 16 == 0 and torch.equal(moved, inside)
    assert host.index_rows(rows.view(6, 4).t()[:4].t()).is_contiguous()
    ws, nbytes = host.workspace(ctypes.c_size_t(48).value, torch.device("cpu"))
    assert nbytes == 48 and ws.dtype == torch.uint8 and ws.numel() == 48
    with host.NO_GUARD:                                                          # the null context is re-enterable: one object serves every call
        with host.NO_GUARD:
            pass


@pytest.mark.parametrize("name", MODULES)
def test_declare_sets_exactly_the_modules_table(name):
    from youreditableavatar_amd import build
    mod = _module(name)
    fresh = ctypes.CDLL(build.build_native())                                    # ctypes caches per handle: a fresh one has nothing declared
    others = set().union(*(set(_module(m).SIGNATURES) for m in MODULES if m != name))
    assert not set(mod.SIGNATURES) & others, name                                # no entry point is in two tables
    assert mod.declare(fresh) is fresh
    for entry, (restype, argtypes) in mod.SIGNATURES.items():
        fn = getattr(fresh, entry)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), (name, entry)
    for entry in others:
        fn = getattr(fresh, entry)
        assert fn.argtypes is None and fn.restype is ctypes.c_int, (name, entry)   # untouched: ctypes' defaults
