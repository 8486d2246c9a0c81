"""Torch CPU restatement of the mesh shading rules (include/tgs_raster.h, "mesh shading"), runnable in float64 and float32.

Scenes and ``rast`` are tests/mesh_ref.py's and tests/mesh_aa_ref.py's (``scene``, ``reference``, ``rast_of`` behind ``scene_rast``); which pixels are
covered is tests/mesh_grad_ref.py's ``covered``.  The smooth part is written in torch on the GATHERED vertex rows (one copy per covered pixel), so
autograd gives the gradients and a leaf copy's ``.grad`` holds the per-pixel contributions, whose largest magnitude B and largest count per
vertex n give the fixed-point term of the header.  The same code run in float32 gives the noise eta.  Nothing here looks at the code under test."""
import numpy as np
import torch

from tests import mesh_grad_ref as G

AMBIGUOUS_CAP = 0.01               # of a scene's covered pixels (tests/mesh_ref.py's cap)
FLIP_MARGIN = 1e-5                 # |m'.z| <= FLIP_MARGIN |m'|: the flip may go either way
SCENES = ("hand_1x1", "hand_7x5", "grid_97x61", "coarse_200x150", "offscreen_40x24", "sphere_256", "fullscreen_512", "tiny_256")
OWN_Z = ("sphere_256", "fullscreen_512")          # their clip z stays away from zero; the others take 2 + z

scene, scene_rast = G.scene, G.scene_rast


def _seed(name, tag):
    return sum(ord(ch) for ch in name + tag) * 8 + len(name)


def normals(name):
    """unit vertex normals, float32 [V,3]: the icosphere's own, otherwise seeded random"""
    s = scene(name)
    if "verts" in s:
        n = np.asarray(s["verts"], np.float64)
    else:
        n = np.random.default_rng(_seed(name, "vn")).normal(size=(len(s["pos"]), 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def rotation(name, tag="rot"):
    """a seeded random rotation, float32 [3,3]"""
    q, r = np.linalg.qr(np.random.default_rng(_seed(name, tag)).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def clip_z(name):
    """the z column a depth test passes, float32 [V]"""
    z = np.asarray(scene(name)["pos"], np.float32)[:, 2]
    return z.copy() if name in OWN_Z else (np.float32(2.0) + z).astype(np.float32)


def inverse3(R):
    """the inverse of a [3,3] tensor by adjugate over determinant, in R's precision"""
    a, b, c, d, e, f, g, h, i = R.reshape(-1)
    A, B, C = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * A + b * B + c * C
    adj = torch.stack([A, c * h - b * i, b * f - c * e, B, a * i - c * g, c * d - a * f, C, b * g - a * h, a * e - b * d]).reshape(3, 3)
    return adj / det


def transformed(VN3, uv, mode, rot, flip):
    """VN3 [n,3,3] the three vertices' normals per pixel, uv [n,2] -> m' [n,3]: the interpolated normal through the mode's transform"""
    m = G.interpolate_torch(VN3, uv)
    if mode == "camera":
        m = m @ inverse3(rot).T
        if flip:
            m = torch.where(m[:, 2:3] < 0, -m, m)
    return m


def shade_torch(VN3, uv, mode, rot, flip, Z3=None):
    """-> (normal [n,3] as stored, depth [n] as stored or None) for the covered pixels"""
    m = transformed(VN3, uv, mode, rot, flip)
    n = torch.nn.functional.normalize(m, dim=-1)                                  # m / max(|m|, 1e-12)
    if mode == "world":
        n = n[:, [1, 2, 0]]
    normal = (n + 1.0) / 2.0
    if Z3 is None:
        return normal, None
    z = G.interpolate_torch(Z3[:, :, None], uv)[:, 0]
    d = 1.0 / (z + 1e-7)
    if len(d) == 0:
        return normal, d
    dmax, dmin = torch.max(d), torch.min(d)
    return normal, (d - dmin) / (dmax - dmin + 1e-7)


def _gather(dtype, rast, tri, vn, zattr):
    rast, vn = np.asarray(rast, np.float32), np.asarray(vn, np.float32)
    pix, vid = G.covered(rast, tri, len(vn))
    VN3 = G._t(vn[vid].reshape(-1, 3, 3), dtype).requires_grad_(True)
    uv = G._t(rast.reshape(-1, 4)[pix][:, :2], dtype).requires_grad_(True)
    Z3 = None if zattr is None else G._t(np.asarray(zattr, np.float32)[vid].reshape(-1, 3), dtype).requires_grad_(True)
    return pix, vid, VN3, uv, Z3


def flip_ambiguous(rast, tri, vn, rot):
    """-> (bool [H,W]: covered pixels with |m'.z| <= FLIP_MARGIN |m'| in camera mode, the number of covered pixels)"""
    rast = np.asarray(rast, np.float32)
    H, W = rast.shape[:2]
    pix, vid, VN3, uv, _ = _gather(torch.float64, rast, tri, vn, None)
    amb = np.zeros(H * W, bool)
    if len(pix):
        with torch.no_grad():
            m = transformed(VN3, uv, "camera", G._t(rot, torch.float64), False)
        amb[pix] = (m[:, 2].abs() <= FLIP_MARGIN * m.norm(dim=1)).numpy()
    return amb.reshape(H, W), len(pix)


def shade(dtype, rast, tri, vn, mode, rot=None, flip=True, zattr=None, g=None):
    """rast [H,W,4], vn [V,3], rot [3,3] (camera mode), zattr [V] or None, g [H,W,C] or None (float32 arrays) -> dict of float64 arrays evaluated in
    ``dtype``: out [H,W,C]; with g also d_vn [V,3], d_z [V] (with zattr), d_rast [H,W,4], and of each scatter B (the largest |per-pixel
    contribution|) and n (the largest number of pixels that reach one vertex): B_vn, B_z, n"""
    rast = np.asarray(rast, np.float32)
    H, W = rast.shape[:2]
    V, C = len(vn), 4 if zattr is None else 5
    pix, vid, VN3, uv, Z3 = _gather(dtype, rast, tri, vn, zattr)
    rot_t = None if rot is None else G._t(rot, dtype)
    normal, depth = shade_torch(VN3, uv, mode, rot_t, flip, Z3)
    out = torch.zeros((H * W, C), dtype=dtype)
    rows = torch.from_numpy(pix)
    parts = [torch.ones((len(pix), 1), dtype=dtype), normal] + ([depth[:, None]] if zattr is not None else [])
    out = out.index_put((rows,), torch.cat(parts, 1))
    res = dict(out=out.detach().double().numpy().reshape(H, W, C), covered=pix)
    if g is None:
        return res
    d_vn, d_z, d_rast = torch.zeros((V, 3), dtype=dtype), torch.zeros((V,), dtype=dtype), np.zeros((H * W, 4))
    res.update(B_vn=0.0, B_z=0.0, n=0)
    if len(pix):
        (out * G._t(np.asarray(g, np.float32).reshape(-1, C), dtype)).sum().backward()
        at = torch.from_numpy(vid.reshape(-1))
        d_vn.index_add_(0, at, VN3.grad.reshape(-1, 3))
        d_rast[pix, :2] = uv.grad.double().numpy()
        res.update(B_vn=float(VN3.grad.abs().max()), n=int(np.bincount(vid.reshape(-1)).max()))
        if Z3 is not None:
            d_z.index_add_(0, at, Z3.grad.reshape(-1))
            res["B_z"] = float(Z3.grad.abs().max())
    res.update(d_vn=d_vn.double().numpy(), d_z=d_z.double().numpy(), d_rast=d_rast.reshape(H, W, 4))
    return res
