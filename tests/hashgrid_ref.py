"""Torch CPU restatement of the hash-grid field's rules (include/tgs_raster.h, "hash-grid field"), differentiated by autograd.

Everything is written in torch on the dtype of ``params``: float64 is the reference, the same code in float32 gives the noise eta.  The float32 run takes
its cell decisions (``floor``) from the float64 run (``cells=``): a point next to a cell face would otherwise land in another cell and inflate eta of the
discontinuous dL_dx for every element.  The box map is an fp32 operation by rule and is evaluated in float32 in both runs.  Nothing here looks at the code
under test: the level table is computed here again, from the config."""
import collections
import functools
import os

import numpy as np
import torch

GRAD_FRAC = 34
MAX_COORD = 1024.0
Level = collections.namedtuple("Level", "scale resolution size offset dense")

CONFIGS = {
    "default": dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.381912879967776),
    "tiny": dict(otype="HashGrid", n_levels=4, n_features_per_level=2, log2_hashmap_size=6, base_resolution=2, per_level_scale=2.0),
    "odd": dict(otype="Grid", type="Hash", n_levels=5, n_features_per_level=2, log2_hashmap_size=8, base_resolution=3, per_level_scale=1.5),
}
_WIDE = dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=7, base_resolution=2, per_level_scale=1.3)
_SINGLE = dict(otype="HashGrid", n_levels=1, n_features_per_level=2, log2_hashmap_size=5, base_resolution=3, per_level_scale=2.0)
CONFIGS.update(wide=_WIDE, wide_thin=_WIDE, single=_SINGLE, single_wide=_SINGLE)      # the launch cases' grids: every table is below 16 KB
MLP = {"default": (64, 1), "tiny": (16, 3), "odd": (32, 4)}           # hidden width and outputs of the fused field in each config's cases
MLP.update(wide=(64, 4), wide_thin=(16, 1), single=(16, 2), single_wide=(64, 4))     # the full LDS layout; most chunks skipped; C = 2 and D = 2
BBOX = ((-1.0, -0.5, -2.0), (1.0, 1.5, 1.0))                           # the box the fused cases map their points from
POINT_SETS = ("uniform", "lattice", "pile", "one", "outside")
CASES = [("default", "uniform"), ("default", "pile")] + [(c, s) for c in ("tiny", "odd") for s in POINT_SETS]   # (the default table is 49 MB)
# The launch cases (tests/test_gpu_hashgrid_launch.py): the shapes at which the kernels take the branches that CASES leaves alone.
LAUNCH_SETS = ("many", "runs", "far")
MANY = 1024 * 256 + 2 * 256 + 77                                       # above HG_MAX_SLABS * HG_BLOCK: workgroups 0, 1, 2 take two tiles, the last a partial one
RUN_LENGTHS = (1, 2, 3, 5, 31, 33, 63, 64, 65, 127, 130, 200, 300)
RUN_REPEATS = 3
NAN_RUN, ZERO_RUN = 70, 13                                             # the run with a NaN row inside, and the run in cell (0,0,0) with one in its middle
FAR_NEAR, FAR_N = 256, 2048
LAUNCH_CASES = [("tiny", "many")] + [(c, s) for c in ("wide", "wide_thin", "single", "single_wide") for s in ("uniform", "runs")] + \
    [(c, "runs") for c in ("tiny", "odd")] + [(c, "far") for c in ("tiny", "odd", "wide")]
KINK_FACTOR = 64.0 * 2.0 ** -24
KINK_CAP = 0.01
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hashgrid_fixture.npz")   # tests/make_ref_hashgrid_fixture.py
FIXTURE_BIAS = 0.125


def fixture():
    return dict(np.load(FIXTURE))


def level_table(config):
    f32 = np.float32
    out, offset = [], 0
    for l in range(config["n_levels"]):
        scale = f32(np.exp2(f32(l) * np.log2(f32(config["per_level_scale"]))) * f32(config["base_resolution"]) - f32(1.0))
        res = int(np.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << config["log2_hashmap_size"])
        out.append(Level(float(scale), res, size, offset, res ** 3 <= size))
        offset += size
    return out


def n_entries(levels):
    return levels[-1].offset + levels[-1].size


def _seed(*names):
    return sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(names)))


def points(config_name, set_name):
    """-> [N,3] float32 in the grid's domain (the unit cube and a little around it; ``far``: up to |x| = 1024).  POINT_SETS and LAUNCH_SETS."""
    rng = np.random.default_rng(_seed(config_name, set_name))
    levels = level_table(CONFIGS[config_name])
    if set_name == "uniform":
        return rng.uniform(0.0, 1.0, (4099, 3)).astype(np.float32)
    if set_name == "lattice":                                           # pos = x scale + 0.5 an integer (up to x's rounding): on the cells' corners
        rows = [np.array([[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)], np.float64)]
        for lv in levels:
            k = rng.integers(1, lv.resolution, (8, 3)).astype(np.float64)
            rows.append((k - 0.5) / max(lv.scale, 1.0))
        return np.concatenate(rows).astype(np.float32)
    if set_name == "pile":
        return np.repeat(rng.uniform(0.0, 1.0, (1, 3)).astype(np.float32), 4096, axis=0)
    if set_name == "one":
        return rng.uniform(0.0, 1.0, (1, 3)).astype(np.float32)
    if set_name == "many":
        return rng.uniform(0.0, 1.0, (MANY, 3)).astype(np.float32)
    if set_name == "runs":
        return _runs(rng, levels[-1].scale)
    if set_name == "far":
        x = np.concatenate([rng.uniform(-3.0, 4.0, (FAR_NEAR, 3)), rng.uniform(-MAX_COORD, MAX_COORD, (FAR_N - FAR_NEAR - 3, 3)), np.zeros((3, 3))]).astype(np.float32)
        x[-3] = (MAX_COORD, -MAX_COORD, MAX_COORD)                       # valid: the rule admits |x| <= 1024
        x[-2] = (0.25, np.nextafter(np.float32(MAX_COORD), np.float32(np.inf)), 0.75)
        x[-1] = (0.5, 0.5, -np.inf)
        return x
    x = rng.uniform(-0.5, 1.5, (17, 3)).astype(np.float32)              # outside
    x[5] = (np.nan, 0.5, 0.5)
    return x


def _runs(rng, scale):
    """consecutive rows in runs of prescribed lengths, each run jittered inside one cell of the finest level (cell k: pos = x scale + 0.5 in [k, k + 1),
    so the centre is x = k / scale, +- 0.2 cell).  RUN_LENGTHS in RUN_REPEATS orders; between them a run of NAN_RUN rows with a NaN row inside, and a
    run of ZERO_RUN rows with every coordinate in [0, 0.5 / scale) -- cell (0,0,0) at every level -- with a NaN row in its middle."""
    def run(n):
        k = rng.integers(1, max(int(np.floor(scale)), 1) + 1, 3).astype(np.float64)
        return (k + rng.uniform(-0.2, 0.2, (n, 3))) / scale
    parts = []
    for rep in range(RUN_REPEATS):
        parts += [run(int(n)) for n in rng.permutation(RUN_LENGTHS)]
        if rep == 0:
            holed = run(NAN_RUN)
            holed[NAN_RUN // 3] = (np.nan, 0.5, 0.5)
            parts.append(holed)
        if rep == 1:
            zero = rng.uniform(0.0, 0.499 / scale, (ZERO_RUN, 3))
            zero[ZERO_RUN // 2] = (0.5, np.nan, 0.5)
            parts.append(zero)
    return np.concatenate(parts).astype(np.float32)


def table(config_name):
    rng = np.random.default_rng(_seed(config_name, "table"))
    return rng.uniform(-0.5, 0.5, 2 * n_entries(level_table(CONFIGS[config_name]))).astype(np.float32)


def weights(config_name):
    rng = np.random.default_rng(_seed(config_name, "weights"))
    H, D = MLP[config_name]
    C = 2 * CONFIGS[config_name]["n_levels"]
    return (rng.uniform(-1.0, 1.0, (H, C)) / np.sqrt(C)).astype(np.float32), (rng.uniform(-1.0, 1.0, (D, H)) / np.sqrt(C)).astype(np.float32)


def upstream(kind, shape, *names):
    rng = np.random.default_rng(_seed(kind, *names) + shape[-1])
    g = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    if kind == "one_row":
        keep = int(rng.integers(0, shape[0]))
        g[np.arange(shape[0]) != keep] = 0.0
    if kind == "binades":                                               # one row 2^40 above the rest: what the bound leaves of the small rows
        keep = int(rng.integers(0, shape[0]))
        g *= np.float32(2.0 ** -20)
        g[keep] *= np.float32(2.0 ** 40)
    if kind == "denormal":                                              # max |g| = 2^-130: the bound is a denormal
        g = (g.astype(np.float64) / np.abs(g).max() * 2.0 ** -130).astype(np.float32)
    return g


def unbox(x):
    """points of the unit cube -> the points of BBOX that the fp32 box map sends (about) there"""
    mn, mx = np.float32(BBOX[0]), np.float32(BBOX[1])
    return (x * (mx - mn) + mn).astype(np.float32)


def box_map(x32, bbox):
    """the rule's fp32 map, every operation rounded on its own"""
    mn, mx = (torch.tensor(b, dtype=torch.float32, device=x32.device) for b in bbox)
    return (x32 - mn) / (mx - mn)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def valid_rows(x):
    return (torch.isfinite(x) & (x.abs() <= MAX_COORD)).all(dim=1)


def corner_indices(cell, lv):
    """cell [N,3] int64 -> the eight corners' entries [N,8] int64, each in [0, size)"""
    M = 0xFFFFFFFF
    out = []
    for i in range(8):
        cx, cy, cz = (cell[:, 0] + (i & 1)) & M, (cell[:, 1] + ((i >> 1) & 1)) & M, (cell[:, 2] + (i >> 2)) & M
        if lv.dense:
            index = (cx + cy * lv.resolution + cz * lv.resolution * lv.resolution) & M
        else:
            index = cx ^ ((cy * 2654435761) & M) ^ ((cz * 805459861) & M)      # (int64 products wrap: the low 32 bits are the uint32 product's)
        out.append(index % lv.size)
    return torch.stack(out, dim=1)


def encode(x, params, levels, active=None, cells=None):
    """x [N,3] and params [2 entries] of one dtype -> (enc [N, 2 n_levels], the cells per level: the decisions a float32 run is given back)"""
    dtype, N = params.dtype, x.shape[0]
    active = len(levels) if active is None else active
    valid = valid_rows(x.detach())
    xs = torch.where(valid[:, None], x, torch.full_like(x, 0.5))
    rows = params.view(-1, 2)
    made, at, wts = [None] * len(levels), [], []
    for l, lv in enumerate(levels[:active]):
        pos = xs * lv.scale + 0.5
        cell = torch.floor(pos.detach()).to(torch.int64) if cells is None else cells[l]
        frac = pos - cell.to(dtype)
        made[l] = cell
        at.append(lv.offset + corner_indices(cell, lv))
        wts.append(torch.stack([(frac[:, 0] if i & 1 else 1.0 - frac[:, 0]) * (frac[:, 1] if i & 2 else 1.0 - frac[:, 1]) * (frac[:, 2] if i & 4 else 1.0 - frac[:, 2])
                                for i in range(8)], dim=1))
    enc = torch.zeros((N, 2 * len(levels)), dtype=dtype, device=x.device)
    if active:                                                                  # one gather of every level's corners: [N, active, 8, 2]
        val = (torch.stack(wts, dim=1)[..., None] * rows[torch.stack(at, dim=1)]).sum(dim=2)
        enc = torch.cat([val.reshape(N, 2 * active), enc[:, 2 * active:]], dim=1)
    return torch.where(valid[:, None], enc, torch.full_like(enc, float("nan"))), made


def field(x32, params, levels, W1, W2, bbox=None, bias=0.0, active=None, cells=None):
    """x32 [N,3] float32 -> (out [N,D], enc, the hidden pre-activations z [N,H], cells) in the dtype of params"""
    xm = (box_map(x32, bbox) if bbox is not None else x32).to(params.dtype)
    enc, cells = encode(xm, params, levels, active, cells)
    valid = valid_rows(xm)[:, None]
    z = torch.where(valid, enc, torch.zeros_like(enc)) @ W1.T                   # a NaN row contributes nothing to any gradient: it leaves before the products
    out = torch.relu(z) @ W2.T + bias
    return torch.where(valid, out, torch.full_like(out, float("nan"))), enc, z, cells


def encode_slow(x, params, levels, active=None):
    """the same rules point by point in Python floats (doubles) -> enc [N, 2 n_levels] as an array; for tests/test_hashgrid_ref.py"""
    active = len(levels) if active is None else active
    out = np.zeros((len(x), 2 * len(levels)))
    for n, p in enumerate(np.asarray(x, np.float32)):
        if not all(np.isfinite(v) and abs(v) <= MAX_COORD for v in p):
            out[n] = np.nan
            continue
        for l, lv in enumerate(levels[:active]):
            pos = [float(v) * lv.scale + 0.5 for v in p]
            cell = [int(np.floor(v)) for v in pos]
            frac = [v - c for v, c in zip(pos, cell)]
            for i in range(8):
                cx, cy, cz = ((cell[0] + (i & 1)) % 2 ** 32, (cell[1] + ((i >> 1) & 1)) % 2 ** 32, (cell[2] + (i >> 2)) % 2 ** 32)
                index = (cx + cy * lv.resolution + cz * lv.resolution ** 2) % 2 ** 32 if lv.dense else cx ^ (cy * 2654435761 % 2 ** 32) ^ (cz * 805459861 % 2 ** 32)
                index %= lv.size
                w = (frac[0] if i & 1 else 1 - frac[0]) * (frac[1] if i & 2 else 1 - frac[1]) * (frac[2] if i & 4 else 1 - frac[2])
                out[n, 2 * l] += w * float(params[2 * (lv.offset + index)])
                out[n, 2 * l + 1] += w * float(params[2 * (lv.offset + index) + 1])
    return out


def most_contributions(x32, levels, active=None):
    """the largest number of (point, corner) contributions that meet in one entry"""
    active = len(levels) if active is None else active
    x = torch.as_tensor(x32)
    x = x[valid_rows(x)].double()
    most = 0
    for lv in levels[:active]:
        if len(x):
            idx = corner_indices(torch.floor(x * lv.scale + 0.5).to(torch.int64), lv)
            most = max(most, int(torch.bincount(idx.reshape(-1), minlength=lv.size).max()))
    return most


def kinked(z64, enc64, W1_64):
    """[N] bool: some hidden pre-activation lies within the fp32 noise of the ReLU's kink, |z_k| < 64 2^-24 sum_j |W1[k,j]| |enc_j|"""
    noise = KINK_FACTOR * (enc64.abs() @ W1_64.abs().T)
    return ((z64.abs() < noise) & torch.isfinite(z64)).any(dim=1)


def field_bound(g, W1, W2):
    """the header's analytic bound of the fused path: max |g| max_j sum_k sum_o |W1[k,j]| |W2[o,k]|, in double"""
    W1, W2 = np.abs(np.asarray(W1, np.float64)), np.abs(np.asarray(W2, np.float64))
    return float(np.abs(np.asarray(g, np.float64)).max()) * float((W1 * W2.sum(axis=0)[:, None]).sum(axis=0).max()) if np.size(g) else 0.0


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().numpy()


def _encode_run(dtype, x32, P, levels, g, active, cells):
    x = torch.tensor(x32).to(dtype).requires_grad_(True)
    p = torch.tensor(P).to(dtype).requires_grad_(True)
    enc, cells = encode(x, p, levels, active, cells)
    valid = valid_rows(torch.tensor(x32))
    (torch.where(valid[:, None], enc, torch.zeros_like(enc)) * torch.tensor(g).to(dtype)).sum().backward()
    return dict(enc=_np(enc), d_params=_np(p.grad), d_x=_np(x.grad)), cells


def _field_run(dtype, x32, P, levels, W1, W2, g, active, cells):
    p, w1, w2 = (torch.tensor(a).to(dtype).requires_grad_(g is not None) for a in (P, W1, W2))
    out, enc, z, cells = field(torch.tensor(x32), p, levels, w1, w2, BBOX, 0.25, active, cells)
    if g is None:
        return None, (enc, z, w1), cells
    valid = valid_rows(box_map(torch.tensor(x32), BBOX))
    (torch.where(valid[:, None], out, torch.zeros_like(out)) * torch.tensor(g).to(dtype)).sum().backward()
    return dict(out=_np(out), d_params=_np(p.grad), d_W1=_np(w1.grad), d_W2=_np(w2.grad)), (enc.detach(), z.detach(), w1.detach()), cells


@functools.lru_cache(maxsize=None)
def case(config_name, set_name, kind="random", active=None):
    """One case, computed once and shared: the inputs (float32 arrays), and for the encoding (``enc``) and the fused field (``fld``) the float64 and
    float32 results, the bound B and the largest count n of the fixed-point term, the valid rows, and the rows the kink rule excludes."""
    levels = level_table(CONFIGS[config_name])
    x, P = points(config_name, set_name), table(config_name)
    W1, W2 = weights(config_name)
    C = 2 * len(levels)
    g_enc = upstream(kind, (len(x), C), config_name, set_name, "enc")
    e64, cells = _encode_run(torch.float64, x, P, levels, g_enc, active, None)
    e32, _ = _encode_run(torch.float32, x, P, levels, g_enc, active, cells)
    xb = unbox(x)
    g_out = upstream(kind, (len(x), MLP[config_name][1]), config_name, set_name, "out")
    _, (enc64, z64, w64), fcells = _field_run(torch.float64, xb, P, levels, W1, W2, None, active, None)
    kinks = kinked(z64, enc64, w64).numpy()
    g_out[kinks] = 0.0                                                         # a point on a kink carries a zero upstream
    f64, _, _ = _field_run(torch.float64, xb, P, levels, W1, W2, g_out, active, fcells)
    f32, _, _ = _field_run(torch.float32, xb, P, levels, W1, W2, g_out, active, fcells)
    xm = box_map(torch.tensor(xb), BBOX)
    out = dict(levels=levels, x=x, xb=xb, params=P, W1=W1, W2=W2, g_enc=g_enc, g_out=g_out, active=active, kinks=kinks,
               valid=valid_rows(torch.tensor(x)).numpy(), valid_b=valid_rows(xm).numpy(),
               enc=dict(ref64=e64, ref32=e32, B=float(np.abs(g_enc).max()), n=most_contributions(x, levels, active)),
               fld=dict(ref64=f64, ref32=f32, B=field_bound(g_out, W1, W2), n=most_contributions(xm.numpy(), levels, active)))
    for a in (x, xb, P, W1, W2, g_enc, g_out):
        a.setflags(write=False)
    return out


def run_lengths(cell, valid, wave=None):
    """the lengths of the runs of consecutive valid rows in one cell ([N,3] int64), an invalid row breaking a run; with ``wave``, a run also ends
    where a wave of that many rows does -> a list of ints"""
    cell, valid = np.asarray(cell), np.asarray(valid)
    out, n = [], 0
    for r in range(len(cell)):
        joins = n > 0 and valid[r] and (cell[r] == cell[r - 1]).all() and (wave is None or r % wave)
        if joins:
            n += 1
            continue
        if n:
            out.append(n)
        n = 1 if valid[r] else 0
    return out + ([n] if n else [])


def term_sums(x, valid, params, g, levels, active=None):
    """The sums of the magnitudes of the terms of the encode path's three results, in float64, for the round-once bars: ``enc`` [N, 2 n_levels] =
    sum_i w_i |row_i|; ``d_x`` [N,3] = sum_l scale_l sum_i (|g_0| |row_i0| + |g_1| |row_i1|) (the corner's two other weights); ``d_params`` =
    per element the sum of w |g| over the contributions that reach it.  ``x`` [N,3] float32, ``valid`` [N] bool: the other rows hold zeros and
    reach no element."""
    valid = torch.tensor(np.asarray(valid))
    x = torch.where(valid[:, None], torch.tensor(np.asarray(x)).double(), torch.full((1, 3), 0.5, dtype=torch.float64))
    rows, g = torch.tensor(np.asarray(params)).double().abs().view(-1, 2), torch.tensor(np.asarray(g)).double().abs() * valid[:, None]
    m_enc, m_x, m_p = torch.zeros_like(g), torch.zeros_like(x), torch.zeros_like(rows)
    for l, lv in enumerate(levels[:len(levels) if active is None else active]):
        pos = x * lv.scale + 0.5
        cell = torch.floor(pos).to(torch.int64)
        f = pos - cell.double()
        at = lv.offset + corner_indices(cell, lv)
        side = [[(f[:, d] if (i >> d) & 1 else 1.0 - f[:, d]) for d in range(3)] for i in range(8)]
        w = torch.stack([a * b * c for a, b, c in side], dim=1) * valid[:, None]                      # [N,8]
        v = rows[at]                                                                                    # [N,8,2]
        gl = g[:, 2 * l:2 * l + 2]
        m_enc[:, 2 * l:2 * l + 2] = (w[..., None] * v).sum(dim=1)
        s = (v * gl[:, None, :]).sum(dim=2)                                                             # [N,8]
        for d in range(3):
            others = torch.stack([side[i][(d + 1) % 3] * side[i][(d + 2) % 3] for i in range(8)], dim=1)
            m_x[:, d] += lv.scale * (s * others).sum(dim=1)
        m_p.index_add_(0, at.reshape(-1), (w[..., None] * gl[:, None, :]).reshape(-1, 2))
    return dict(enc=m_enc.numpy(), d_x=m_x.numpy(), d_params=m_p.reshape(-1).numpy())


@functools.lru_cache(maxsize=None)
def magnitudes(config_name, set_name, kind="random", active=None):
    """``term_sums`` of a case's encode path, computed once"""
    c = case(config_name, set_name, kind, active)
    return term_sums(c["x"], c["valid"], c["params"], c["g_enc"], c["levels"], active)
