"""NumPy restatement of the mesh rasterizer's rule (include/tgs_raster.h, "mesh rasterizer"), and the scenes its tests use.

Coverage is decided in int64 on vertices snapped in float64; depth, u and v are evaluated in float64.  A second evaluation of the float part
in float32 -- the same sequence of operations -- measures the arithmetic's own noise: eta_z and eta_uv are the largest |fp32 - fp64| over
pixels where both evaluations pick the same winner.  Nothing here looks at the code under test.

Scene generators keep the snapping unambiguous: every vertex's subpixel coordinate, evaluated in fp64, lies farther from a half-integer than
12 * 2^-24 * max|X| (six fp32 roundings on a magnitude of max|X|, doubled); offending vertices are nudged and the result is asserted."""
import functools

import numpy as np

SNAP_MAX = float(2 ** 29)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def snap(pos, W, H):
    """-> X, Y (int64 [V]) and ok (bool [V]: w > 0, finite, |X|, |Y| <= 2^29), plus the unrounded fp64 subpixel coordinates"""
    p = np.asarray(pos, np.float64)
    with np.errstate(all="ignore"):
        fx = (p[:, 0] / p[:, 3] * 0.5 + 0.5) * W * 256.0
        fy = (p[:, 1] / p[:, 3] * 0.5 + 0.5) * H * 256.0
    ok = np.isfinite(p).all(axis=1) & (p[:, 3] > 0)
    fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
    rx, ry = np.rint(fx), np.rint(fy)
    ok &= (np.abs(rx) <= SNAP_MAX) & (np.abs(ry) <= SNAP_MAX)
    return np.where(ok, rx, 0).astype(np.int64), np.where(ok, ry, 0).astype(np.int64), ok, fx, fy


def _candidates(X, Y, ok, tri, W, H, window):
    """every (triangle, pixel) pair of the triangles' pixel boxes, clamped to the window: -> t, i, j (int64)"""
    x0, y0, x1, y1 = window
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    good = ok[tri].all(axis=1) if len(tri) else np.zeros(0, bool)
    tx, ty = X[tri], Y[tri]
    # pixel i can be inside only if Xmin <= 256 i + 128 <= Xmax
    bx0 = np.maximum(x0, -((-(tx.min(1) - 128)) // 256)); bx1 = np.minimum(x1 - 1, (tx.max(1) - 128) // 256)
    by0 = np.maximum(y0, -((-(ty.min(1) - 128)) // 256)); by1 = np.minimum(y1 - 1, (ty.max(1) - 128) // 256)
    good &= (bx0 <= bx1) & (by0 <= by1)
    ids = np.nonzero(good)[0]
    nx, ny = (bx1 - bx0 + 1)[ids], (by1 - by0 + 1)[ids]
    cnt = nx * ny
    t = np.repeat(ids, cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    nxr = np.repeat(nx, cnt)
    return t, np.repeat(bx0[ids], cnt) + k % nxr, np.repeat(by0[ids], cnt) + k // nxr


def covered(X, Y, tri, t, i, j):
    """the integer rule for the pairs (t, i, j): orientation by sign(A), E > 0 or E = 0 on an owning edge"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    vx, vy = X[tri[t]], Y[tri[t]]                                       # [n,3]
    A = (vx[:, 1] - vx[:, 0]) * (vy[:, 2] - vy[:, 0]) - (vx[:, 2] - vx[:, 0]) * (vy[:, 1] - vy[:, 0])
    sgn = np.sign(A)
    Px, Py = 256 * i + 128, 256 * j + 128
    inside = A != 0
    for a, b in ((0, 1), (1, 2), (2, 0)):
        dx, dy = sgn * (vx[:, b] - vx[:, a]), sgn * (vy[:, b] - vy[:, a])             # the edge of the ORIENTED triangle runs the other way for sgn < 0
        E = sgn * ((vx[:, b] - vx[:, a]) * (Py - vy[:, a]) - (vy[:, b] - vy[:, a]) * (Px - vx[:, a]))
        owner = (dy < 0) | ((dy == 0) & (dx > 0))
        inside &= (E > 0) | ((E == 0) & owner)
    return inside


def float_part(dtype, pos, tri, t, i, j, W, H):
    """z/w, u, v of the pairs (t, i, j) in ``dtype`` arithmetic, one rounding per operation, in the order csrc/tgs_mesh.hip writes them"""
    f = dtype
    p = np.asarray(pos, np.float32).astype(f)[np.asarray(tri, np.int64).reshape(-1, 3)[t]]         # [n,3,4]
    half, one = f(0.5), f(1.0)
    with np.errstate(all="ignore"):
        sx = (p[:, :, 0] / p[:, :, 3] * half + half) * f(W)
        sy = (p[:, :, 1] / p[:, :, 3] * half + half) * f(H)
        zw = p[:, :, 2] / p[:, :, 3]
        iw = one / p[:, :, 3]
        e1x, e1y, e2x, e2y = sx[:, 1] - sx[:, 0], sy[:, 1] - sy[:, 0], sx[:, 2] - sx[:, 0], sy[:, 2] - sy[:, 0]
        inv = one / (e1x * e2y - e1y * e2x)
        px, py = (i.astype(f) + half) - sx[:, 0], (j.astype(f) + half) - sy[:, 0]
        b1 = (px * e2y - py * e2x) * inv
        b2 = (e1x * py - e1y * px) * inv
        z = (zw[:, 0] + b1 * (zw[:, 1] - zw[:, 0])) + b2 * (zw[:, 2] - zw[:, 0])
        b0 = (one - b1) - b2
        q0, q1, q2 = b0 * iw[:, 0], b1 * iw[:, 1], b2 * iw[:, 2]
        d = (q0 + q1) + q2
        u, v = np.clip(q0 / d, f(0), one), np.clip(q1 / d, f(0), one)
        s = np.maximum(u + v, one)
        u, v = u / s, v / s
    assert z.dtype == f and u.dtype == f
    return z, u, v


def _winners(pix, z, t, n_pix):
    """per pixel the fragment with the smallest (z, t) and the runner-up: -> first, second (indices into the fragment arrays, -1: none)"""
    order = np.lexsort((t, z, pix))
    sp = pix[order]
    start = np.ones(len(sp), bool); start[1:] = sp[1:] != sp[:-1]
    first = np.full(n_pix, -1, np.int64); second = np.full(n_pix, -1, np.int64)
    first[sp[start]] = order[start]
    is2 = np.zeros(len(sp), bool); is2[1:] = start[:-1] & ~start[1:]
    second[sp[is2]] = order[is2]
    return first, second


def rasterize(pos, tri, W, H, window=None):
    """The rule on the pixels of ``window`` = (x0, y0, x1, y1) (default: the whole image).  -> dict of [h,w] maps over the window:
    winner (int64 triangle index, -1: empty), second (the runner-up's index, -1: none), z, z_second (fp64; inf where there is none), u, v
    (fp64, of the winner), and the scalars eta_z, eta_uv, n_same (pixels where the fp32 and fp64 evaluations pick the same winner)."""
    window = (0, 0, W, H) if window is None else tuple(int(x) for x in window)
    x0, y0, x1, y1 = window
    w, h = x1 - x0, y1 - y0
    pos, tri = np.asarray(pos, np.float32).reshape(-1, 4), np.asarray(tri, np.int64).reshape(-1, 3)
    out = dict(winner=np.full((h, w), -1, np.int64), second=np.full((h, w), -1, np.int64), z=np.zeros((h, w)), z_second=np.full((h, w), np.inf),
               u=np.zeros((h, w)), v=np.zeros((h, w)), eta_z=0.0, eta_uv=0.0, n_same=0, window=window)
    if len(tri) == 0 or len(pos) == 0:
        return out
    X, Y, ok, _, _ = snap(pos, W, H)
    t, i, j = _candidates(X, Y, ok, tri, W, H, window)
    keep = covered(X, Y, tri, t, i, j)
    t, i, j = t[keep], i[keep], j[keep]
    z64, u64, v64 = float_part(np.float64, pos, tri, t, i, j, W, H)
    z32, u32, v32 = float_part(np.float32, pos, tri, t, i, j, W, H)
    pix = (j - y0) * w + (i - x0)
    in64, in32 = (z64 >= -1.0) & (z64 <= 1.0), (z32 >= np.float32(-1.0)) & (z32 <= np.float32(1.0))
    idx64 = np.nonzero(in64)[0]
    if len(idx64) == 0 or not in32.any():
        return out
    f64, s64 = _winners(pix[idx64], z64[idx64], t[idx64], h * w)
    idx32 = np.nonzero(in32)[0]
    f32, _ = _winners(pix[idx32], z32[idx32], t[idx32], h * w)
    f64g = np.where(f64 >= 0, idx64[np.maximum(f64, 0)], -1)
    s64g = np.where(s64 >= 0, idx64[np.maximum(s64, 0)], -1)
    f32g = np.where(f32 >= 0, idx32[np.maximum(f32, 0)], -1)
    hit = f64g >= 0
    flat = lambda fill, src, idx: np.where(idx >= 0, src[np.maximum(idx, 0)], fill).reshape(h, w)
    out["winner"], out["second"] = flat(-1, t, f64g), flat(-1, t, s64g)
    out["z"], out["z_second"] = flat(0.0, z64, f64g), flat(np.inf, z64, s64g)
    out["u"], out["v"] = flat(0.0, u64, f64g), flat(0.0, v64, f64g)
    same = hit & (f32g == f64g)
    g = f64g[same]
    out["n_same"] = int(same.sum())
    if len(g):
        out["eta_z"] = float(np.abs(z32[g].astype(np.float64) - z64[g]).max())
        out["eta_uv"] = float(max(np.abs(u32[g].astype(np.float64) - u64[g]).max(), np.abs(v32[g].astype(np.float64) - v64[g]).max()))
    return out


def ambiguous(ref, tri):
    """pixels whose best and second-best fp64 depth are within 4 eta_z.  A runner-up that IS the winner once more (the same three vertex
    indices in the same order: the same bits in any arithmetic) is decided by the index rule and is not ambiguous."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    close = (ref["winner"] >= 0) & (ref["second"] >= 0) & (ref["z_second"] - ref["z"] <= 4.0 * ref["eta_z"])
    if len(tri):
        close &= ~(tri[np.maximum(ref["winner"], 0)] == tri[np.maximum(ref["second"], 0)]).all(axis=-1)
    return close


def interpolate(attr, rast, tri):
    """fp64 evaluation of u a0 + v a1 + (1 - u - v) a2 from a given rast [...,4] -> (out [...,C], bound [...,C]: 8 * 2^-24 * the sum of the
    three products' magnitudes -- three products, two sums and the subtraction)"""
    attr, rast, tri = np.asarray(attr, np.float64), np.asarray(rast, np.float64), np.asarray(tri, np.int64).reshape(-1, 3)
    ids = rast[..., 3].astype(np.int64)
    hit = ids > 0
    vid = tri[np.maximum(ids - 1, 0)] if len(tri) else np.zeros(ids.shape + (3,), np.int64)
    u, v = rast[..., 0:1], rast[..., 1:2]
    if len(attr) == 0:
        z = np.zeros(ids.shape + (attr.shape[-1],))
        return z, z
    t0, t1, t2 = u * attr[vid[..., 0]], v * attr[vid[..., 1]], (1.0 - u - v) * attr[vid[..., 2]]
    out = np.where(hit[..., None], t0 + t1 + t2, 0.0)
    bound = np.where(hit[..., None], 8.0 * 2.0 ** -24 * (np.abs(t0) + np.abs(t1) + np.abs(t2)), 0.0)
    return out, bound


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def clip_from_pixels(px, py, zw, w, W, H):
    """clip-space float32 [V,4] of vertices given in pixel coordinates (pixel (i, j) has its centre at (i + 0.5, j + 0.5)), z/w and w"""
    px, py, zw, w = (np.asarray(a, np.float64) for a in (px, py, zw, w))
    return np.stack([(px / W * 2.0 - 1.0) * w, (py / H * 2.0 - 1.0) * w, zw * w, w], 1).astype(np.float32)


def snap_margin(pos, W, H):
    """-> (distance of every usable vertex's fp64 subpixel coordinates from the nearest half-integer [V,2], the distance required)"""
    _, _, ok, fx, fy = snap(pos, W, H)
    c = np.stack([fx, fy], 1)
    dist = np.abs(c - np.floor(c) - 0.5)
    dist[~ok] = 0.5
    need = 12.0 * 2.0 ** -24 * max(float(np.abs(c[ok]).max()) if ok.any() else 0.0, 1.0)
    return dist, need


def unambiguous(pos, W, H):
    """nudges (by 0.11 subpixel steps in clip space) the vertices whose snapping fp32 and fp64 could decide differently; asserts the result"""
    pos = np.array(pos, np.float32)
    for _ in range(40):
        dist, need = snap_margin(pos, W, H)
        bad = dist <= need
        if not bad.any():
            break
        for axis, size in ((0, W), (1, H)):
            rows = np.nonzero(bad[:, axis])[0]
            step = (0.11 / 256.0) * 2.0 / size * pos[rows, 3].astype(np.float64)
            pos[rows, axis] = (pos[rows, axis].astype(np.float64) + step).astype(np.float32)
    dist, need = snap_margin(pos, W, H)
    assert (dist > need).all(), "a vertex still snaps ambiguously"
    return pos


def hand_scene(W, H):
    """The hand-computed cases in one mesh, for any W x H.  Pixel coordinates are multiples of 1/4, so every snapped coordinate is exact.
    faces 0, 1   a quad [0.5, qx] x [0.5, qy] whose edges pass exactly through pixel centres, as two triangles of OPPOSITE winding, z/w 0.25;
                 it covers exactly the pixels 0 <= i < qx - 0.5, 0 <= j < qy - 0.5 (left / bottom edges own their centres, right / top do not)
    face 2       zero area (a repeated vertex);  face 3  three collinear vertices
    faces 4, 5   screen-filling, but with a vertex at w = -1 / at w = 0: dropped whole
    faces 6, 7   screen-filling at z/w = -1.5 / +1.5: every fragment discarded
    face 8       screen-filling at z/w = 0.5, perspective (w = 1, 2, 0.5): the background of the quad
    faces 9, 10  faces 0 and 1 once more: the lower index wins
    -> pos, tri, (qx, qy)"""
    qx, qy = max(1, W // 2) + 0.5, max(1, H // 2) + 0.5
    big = [(-W - 1.25, -H - 0.75), (5 * W + 0.25, -H - 0.75), (-W - 1.25, 5 * H + 0.5)]
    px = [0.5, qx, qx, 0.5, 0.5 * (0.5 + qx)] + [b[0] for b in big] * 5
    py = [0.5, 0.5, qy, qy, 0.5 * (0.5 + qy)] + [b[1] for b in big] * 5
    zw = [0.25] * 5 + [0.0] * 3 + [0.0] * 3 + [-1.5] * 3 + [1.5] * 3 + [0.5] * 3
    w = [1.0, 2.0, 0.5, 1.5, 1.0] + [1.0, 1.0, 1.0] + [1.0, 1.0, 1.0] + [1.0] * 6 + [1.0, 2.0, 0.5]
    pos = clip_from_pixels(px, py, zw, w, W, H)
    pos[5, 3] = -1.0                                                     # face 4: a vertex behind the camera
    pos[8, 3] = 0.0                                                      # face 5: a vertex at w = 0
    tri = np.array([[0, 1, 2], [0, 3, 2], [0, 0, 1], [0, 4, 2], [5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16], [17, 18, 19], [0, 1, 2], [0, 3, 2]], np.int32)
    return unambiguous_check(pos, W, H), tri, (qx, qy)


def unambiguous_check(pos, W, H):
    dist, need = snap_margin(pos, W, H)
    assert (dist > need).all()
    return pos


def grid_scene(W, H, nx, ny, seed, overhang=2.0, jitter=0.3, w_range=(0.5, 4.0), z=lambda x, y: 0.3 * x - 0.2 * y, flip=True):
    """A jittered nx x ny-cell sheet that overhangs the W x H screen by ``overhang`` cells, two triangles per cell with a random diagonal and (``flip``)
    random windings, random w per vertex; z/w = z(x, y) of the NDC position.  Watertight: it leaves no empty pixel."""
    rng = np.random.default_rng(seed)
    cx, cy = W / (nx - 2 * overhang), H / (ny - 2 * overhang)
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    px = (gx - overhang) * cx + rng.uniform(-jitter, jitter, gx.shape) * cx
    py = (gy - overhang) * cy + rng.uniform(-jitter, jitter, gy.shape) * cy
    px, py = px.reshape(-1), py.reshape(-1)
    w = rng.uniform(w_range[0], w_range[1], px.shape)
    pos = unambiguous(clip_from_pixels(px, py, z(px / W * 2 - 1, py / H * 2 - 1), w, W, H), W, H)
    v = lambda a, b: (b * (nx + 1) + a)
    a, b = np.meshgrid(np.arange(nx), np.arange(ny))
    a, b = a.reshape(-1), b.reshape(-1)
    v00, v10, v11, v01 = v(a, b), v(a + 1, b), v(a + 1, b + 1), v(a, b + 1)
    diag = rng.integers(0, 2, len(a)).astype(bool)
    t1 = np.where(diag[:, None], np.stack([v00, v10, v11], 1), np.stack([v00, v10, v01], 1))
    t2 = np.where(diag[:, None], np.stack([v00, v11, v01], 1), np.stack([v10, v11, v01], 1))
    tri = np.stack([t1, t2], 1).reshape(-1, 3)
    if flip:
        f = rng.integers(0, 2, len(tri)).astype(bool)
        tri[f] = tri[f][:, [0, 2, 1]]
    return pos, tri.astype(np.int32)


def _join(parts):
    pos, tri, off = [], [], 0
    for p, t in parts:
        pos.append(p); tri.append(t + off); off += len(p)
    return np.concatenate(pos).astype(np.float32), np.concatenate(tri).astype(np.int32)


def sphere_scene(W=256, H=256, subdivisions=4):
    """the icosphere (5 120 faces) through a perspective orbit camera: front faces in front of back faces, both windings rasterize"""
    from youreditableavatar_amd import scenes
    verts, faces = scenes.icosphere(subdivisions)
    cam = scenes.orbit_camera(W, H, azimuth_deg=25.0, elevation_deg=15.0, radius=3.0, znear=1.0, zfar=10.0)
    clip = np.concatenate([verts, np.ones((len(verts), 1), np.float32)], 1) @ cam.projmatrix
    return unambiguous(clip.astype(np.float32), W, H), faces, verts


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(pos, tri, W, H, window, ...): every scene the GPU tests rasterize, built once"""
    if name.startswith("hand_"):
        W, H = (int(x) for x in name[5:].split("x"))
        pos, tri, q = hand_scene(W, H)
        return dict(pos=pos, tri=tri, W=W, H=H, window=None, quad=q)
    if name == "grid_97x61":
        pos, tri = grid_scene(97, 61, 24, 16, seed=11)
        return dict(pos=pos, tri=tri, W=97, H=61, window=None)
    if name == "sheets_64x48":
        a = grid_scene(64, 48, 12, 10, seed=21, z=lambda x, y: 0.4 * (x + 0.013) + 0.1 * y)
        b = grid_scene(64, 48, 9, 13, seed=22, z=lambda x, y: -0.4 * (x + 0.013) - 0.05 * y)
        pos, tri = _join([a, b])
        return dict(pos=pos, tri=tri, W=64, H=48, window=None)
    if name == "coarse_200x150":                                                            # about 40 triangles of 60-pixel cells: several regions each
        pos, tri = grid_scene(200, 150, 5, 4, seed=41, overhang=0.5, z=lambda x, y: 0.2 * x + 0.3 * y)
        return dict(pos=pos, tri=tri, W=200, H=150, window=None)
    if name == "offscreen_40x24":
        W, H = 40, 24
        ndc = np.array([[-50, -50], [50, -50], [0.3, 50],                                   # vertices at +-50 NDC: covers the screen
                        [1.5, 1.5], [3.0, 1.5], [1.5, 4.0], [-9, -0.5], [-2, 0.5], [-5, 3], [-0.5, -30], [0.5, -30], [0, -2],      # fully off-screen
                        [-0.6, -0.7], [0.8, -0.2], [0.1, 0.9]], np.float64)                  # one ordinary triangle in front
        w = np.array([1, 2, 0.7, 1, 1, 1, 2, 2, 2, 0.5, 0.5, 0.5, 1.5, 1, 3], np.float64)
        zw = np.array([0.6, 0.7, 0.5] + [0.0] * 9 + [0.1, 0.2, -0.3], np.float64)
        pos = np.stack([ndc[:, 0] * w, ndc[:, 1] * w, zw * w, w], 1).astype(np.float32)
        tri = np.arange(15, dtype=np.int32).reshape(5, 3)
        return dict(pos=unambiguous(pos, W, H), tri=tri, W=W, H=H, window=None)
    if name == "sphere_256":
        pos, tri, verts = sphere_scene()
        return dict(pos=pos, tri=tri, W=256, H=256, window=None, verts=verts)
    if name == "tiny_256":                                                                  # 70 312 triangles of about 1.4 pixels: IDs above 16 bits
        pos, tri = grid_scene(256, 256, 188, 187, seed=31, overhang=1.0, jitter=0.25, w_range=(0.8, 1.6))
        assert len(tri) >= 70000
        return dict(pos=pos, tri=tri, W=256, H=256, window=None)
    if name == "quad_2048":                                                                 # index arithmetic: compared on a crop at the far corner
        W = H = 2048
        pos = unambiguous(clip_from_pixels([3.3, 2040.6, 2044.2, 1.7], [2.4, 5.1, 2045.3, 2041.9], [0.1, 0.3, 0.5, 0.2], [1.0, 2.0, 1.5, 0.8], W, H), W, H)
        return dict(pos=pos, tri=np.array([[0, 1, 2], [0, 2, 3]], np.int32), W=W, H=H, window=(1984, 1990, 2048, 2048))
    if name == "fullscreen_512":                                                            # the large-triangle path: a pair that covers the screen
        W = H = 512
        pos = unambiguous(clip_from_pixels([-3.3, 515.6, 517.2, -1.7], [-2.4, -5.1, 514.3, 516.9], [0.1, 0.3, 0.5, 0.2], [1.0, 2.0, 1.5, 0.8], W, H), W, H)
        return dict(pos=pos, tri=np.array([[0, 1, 2], [0, 2, 3]], np.int32), W=W, H=H, window=None)
    raise KeyError(name)


HAND_SIZES = ("1x1", "7x5", "16x16", "33x17")
GPU_SCENES = tuple("hand_" + s for s in HAND_SIZES) + ("grid_97x61", "sheets_64x48", "coarse_200x150", "offscreen_40x24", "sphere_256", "tiny_256", "quad_2048", "fullscreen_512")
AMBIGUOUS_CAP = 0.01           # of a scene's covered pixels


@functools.lru_cache(maxsize=None)
def reference(name):
    """the rule on scene ``name`` (computed once, read-only)"""
    s = scene(name)
    ref = rasterize(s["pos"], s["tri"], s["W"], s["H"], s["window"])
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref
