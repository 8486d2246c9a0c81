"""The orchestration of SyncFreeBatch.run_views, pinned: which native functions it calls, in which order, with which scalars and which
optional per-view pointers set; on which lane each upstream callable runs; where on_chunk falls between the launches.  The numeric suites
would still pass if a kernel ran for a None gradient, if on_chunk moved relative to the launches, or if a view's loss ran on another lane.

The call goes through a forwarding proxy in place of ``multiview._C`` that logs every function called through it; the upstream callables and
on_chunk log into the same list.  An event per native call: its name, its int / bool / float scalars as they are, tensors and raw pointers
only as present or None, a list of stream handles as its length, a per-view ctypes array as, per view, the optional pointer fields that are
non-null.  The expected logs are tests/golden/run_views_calls.json, written by ``python tests/test_gpu_run_views_calls.py --record`` from
the tree before the orchestration was consolidated; a capacity or a tile bound in them comes from the same library and scene on both sides.

Scene: tests.test_gpu_batch_backward.make_scene at the H, W of tests/test_gpu_batch_extras.py, V = 3 (4 with split lanes), P = 700 --
grad_chunks=2 gives the ranges (0, 512) and (512, 188) -- granule=64, deterministic=True.  Per mode and kind of callable, on one
SyncFreeBatch: the first call (synchronous route); a pooled call with accumulate=False, grad_chunks=2 and on_chunk; a pooled call with
accumulate=True; median_views() and backward_median_views with view 1's entry None; after ``bound = 1`` a call whose views are all
rejected, with on_chunk; median_views() again.  "One view's extra gradient None" is what the view callable returns for that view; the batch
callable has one gradient for all views, so it returns None for that map in the calls without on_chunk."""
import ctypes
import difflib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_batch_backward import _leaves, _settings, _t, make_scene
from tests.test_gpu_batch_extras import H, W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(util.GOLDEN_DIR, "run_views_calls.json")
P, SEED, SCALE_MULT, C_FEAT = 700, 1406, 2.0, 3
OPTIONAL_FIELDS = ("dL_dpix", "dL_dcolor", "out_alpha", "out_depth", "dL_dalpha", "dL_ddepth", "dz_scratch", "out_features", "dL_dfeature_map",
                   "feature_scratch", "out_pos", "dL_dmedian_depth")
MODES = ("sh", "precomp", "alpha_depth", "features_grad", "alpha_features_nograd")
CASES = [(mode, kind, "default") for mode in MODES for kind in ("batch", "view")] + [(mode, "view", "split4") for mode in MODES]
case_id = lambda case: "-".join(case)


def _value(a):
    """an argument of a native call as the log keeps it"""
    if a is None or isinstance(a, (bool, float, str)):
        return a
    if isinstance(a, int):
        return a if abs(a) < (1 << 32) else "ptr"          # (device addresses and stream handles; every scalar of the scene is far below)
    if torch.is_tensor(a):
        return "tensor"
    if isinstance(a, ctypes.Array):
        return {"views": [[f for f in OPTIONAL_FIELDS if getattr(x, f, None)] for x in a]}
    if isinstance(a, (list, tuple)):
        return {"handles": len(a)} if all(isinstance(x, int) for x in a) else [_value(x) for x in a]
    if isinstance(a, dict):
        return {"keys": sorted(a)}
    return type(a).__name__


class _Proxy:
    """stands in for multiview._C: forwards everything, logs the calls"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if not callable(attr) or isinstance(attr, type):
            return attr

        def call(*args, **kwargs):
            self._log.append({"call": name, "args": [_value(a) for a in args], "kwargs": {k: _value(v) for k, v in sorted(kwargs.items())}})
            return attr(*args, **kwargs)
        return call


def _scene(mode, V, dev):
    from youreditableavatar_amd.multiview import FlatGradients
    M = 0 if mode == "precomp" else 16
    cloud, cams, dLs = make_scene(P, V, 1, M, False, SEED, SCALE_MULT, False)
    names = ("means3D", "opacities", "scales", "rotations") + (("shs",) if M else ())
    L = _leaves(cloud, dev, names)
    flat = FlatGradients([L[n] for n in names])
    rng = np.random.Generator(np.random.PCG64(77))
    small = lambda *shape: _t(rng.standard_normal(shape) / (H * W), dev)
    s = dict(L=L, flat=flat, settings=[_settings(c, 1, dev) for c in cams], V=V,
             colors=None if M else torch.stack([_t(util.scene_input(cloud, c, "precomp")["colors_precomp"], dev) for c in cams]),
             dL=torch.stack([_t(d, dev) for d in dLs]), alpha=small(V, 1, H, W), depth=small(V, 1, H, W), features=small(V, C_FEAT, H, W),
             median=small(V, 1, H, W))
    s["maps"] = {"sh": [], "precomp": [], "alpha_depth": ["alpha", "depth"], "features_grad": ["features"], "alpha_features_nograd": ["alpha", "features"]}[mode]
    s["absent"] = {"alpha_depth": ("depth", 1), "features_grad": ("features", 0)}.get(mode)      # (map, view) whose gradient is None
    s["kw"] = dict(return_alpha="alpha" in s["maps"], return_depth="depth" in s["maps"])
    if "features" in s["maps"]:
        F = _t(rng.standard_normal((P, C_FEAT)), dev)
        if mode == "features_grad":
            F.requires_grad_(True)
            F.grad = torch.zeros_like(F)
        s["kw"]["features"] = F
    return s


def record_case(mode, kind, config, dev):
    """the log of the whole sequence of one case"""
    from youreditableavatar_amd import multiview
    s = _scene(mode, 4 if config == "split4" else 3, dev)
    V, L = s["V"], s["L"]
    batch = multiview.SyncFreeBatch(granule=64, deterministic=True, **(dict(split=True, streams=4) if config == "split4" else {}))
    log, step = [], {}

    def lane():
        main = step["main"]
        return multiview._lanes(main, batch.streams).index(torch.cuda.current_stream(main.device))

    def grads(v):
        """the upstream callable's return for view v (None: the batch)"""
        out = []
        for name in s["maps"]:
            absent = s["absent"] is not None and s["absent"][0] == name and (s["absent"][1] == v if v is not None else step["accumulate"])
            out.append(None if absent else (s[name] if v is None else s[name][v]))
        dL = s["dL"] if v is None else s["dL"][v]
        return (dL, *out) if s["maps"] else dL

    def upstream_batch(images, *maps):
        log.append({"call": "upstream_batch", "lane": lane(), "maps": len(maps)})
        return grads(None)

    def upstream_view(v, image, *maps):
        log.append({"call": "upstream_view", "v": v, "lane": lane(), "maps": len(maps)})
        return grads(v)

    def on_chunk(first, count):
        log.append({"call": "on_chunk", "first": first, "count": count})

    def run(what, accumulate=True, **kw):
        log.append({"call": "--", "step": what})
        step.update(main=torch.cuda.current_stream(dev), accumulate=accumulate and "on_chunk" not in kw)
        ups = (upstream_batch,) if kind == "batch" else (None,)
        out = batch.run_views(s["settings"], L["means3D"], L["opacities"], L.get("shs"), L["scales"], L["rotations"], *ups, accumulate=accumulate,
                              colors_precomp=s["colors"], upstream_view=upstream_view if kind == "view" else None, **s["kw"], **kw)
        assert (len(out) == 1 + len(s["maps"])) if s["maps"] else torch.is_tensor(out)

    def median(what, backward):
        log.append({"call": "--", "step": what})
        depth, index = batch.median_views()
        assert tuple(depth.shape) == tuple(index.shape) == (V, 1, H, W)
        if backward:
            batch.backward_median_views([None if v == 1 else s["median"][v] for v in range(V)])

    real, multiview._C = multiview._C, _Proxy(multiview._C, log)
    try:
        s["flat"].zero_()
        run("first call")
        assert batch.capacity() is not None
        run("pooled, stored, two ranges", accumulate=False, grad_chunks=2, on_chunk=on_chunk)
        run("pooled, accumulated")
        assert batch.rejected == 0
        median("median and its gradient", True)
        batch.bound = 1                                     # capacity 64: below every view's instance count
        run("every view rejected", grad_chunks=2, on_chunk=on_chunk)
        assert batch.rejected == V
        median("median of re-rendered views", False)
        torch.cuda.synchronize()
    finally:
        multiview._C = real
    return json.loads(json.dumps(log))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode,kind,config", CASES, ids=[case_id(c) for c in CASES])
def test_run_views_makes_the_recorded_calls(mode, kind, config, golden, gpu_device):
    want = golden[case_id((mode, kind, config))]
    got = record_case(mode, kind, config, gpu_device)
    if got != want:
        lines = lambda log: [json.dumps(e, sort_keys=True) for e in log]
        diff = "\n".join(difflib.unified_diff(lines(want), lines(got), "recorded", "this tree", lineterm="", n=2))
        pytest.fail(f"{case_id((mode, kind, config))}: the calls differ from the recorded ones\n{diff}", pytrace=False)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_run_views_calls.py --record [FILE]")
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    logs = {case_id(c): record_case(*c, torch.device("cuda:0")) for c in CASES}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join("  " + json.dumps(e, sort_keys=True) for e in log) + "\n]"
                                   for k, log in logs.items()) + "\n}\n")
    print("wrote", out, {k: len(v) for k, v in logs.items()})
