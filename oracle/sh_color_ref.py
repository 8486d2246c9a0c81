"""CPU restatement of TetGS.get_points_rgb (TEST INFRASTRUCTURE ONLY): Edit_core/tetgs_scene/tetgs_model.py:413-442
with eval_sh of Edit_core/utils/spherical_harmonics.py:117-172, in plain PyTorch so autograd gives the gradients.
Pinned by tests/golden/ref_utils_fixture.npz (outputs and gradients of the reference's own eval_sh)."""
import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def eval_sh(deg, sh, dirs):
    """sh [..., C, (deg+1)^2], dirs [..., 3] (spherical_harmonics.py:117-172, degrees 0-3)."""
    result = C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        result = result - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            result = (result + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
                      + C2[3] * xz * sh[..., 7] + C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                result = (result + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10]
                          + C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
                          + C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + C3[5] * z * (xx - yy) * sh[..., 14]
                          + C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return result


def points_rgb(sh_coordinates, sh_levels, positions=None, camera_centers=None, directions=None):
    """tetgs_model.py:413-442."""
    if camera_centers is not None:
        render_directions = torch.nn.functional.normalize(positions - camera_centers, dim=-1)
    elif directions is not None:
        render_directions = directions
    else:
        raise ValueError("Either camera_centers or directions must be provided.")
    sh = sh_coordinates[:, :sh_levels ** 2]
    shs_view = sh.transpose(-1, -2).reshape(-1, 3, sh_levels ** 2)
    sh2rgb = eval_sh(sh_levels - 1, shs_view, render_directions)
    return torch.clamp_min(sh2rgb + 0.5, 0.0).view(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Row-by-row comparison of the fused kernels (tests/test_sh_color_matrix.py).  Everything below is evaluated in float64 from the reference
# above: the bars are first-order rounding bounds against scales that cancellation cannot shrink, not measurements of the code under test.
U = 2.0 ** -24                  # unit roundoff of fp32
COLOR_U, DSH_U, DDIR_U = 32.0, 32.0, 128.0
PRE_BLOCK = 256                 # Gaussians per workgroup of k_sh_rgb / k_sh_rgb_dcrest (csrc/tgs_device.hpp)


def dcrest_path(P, Mr, levels, aligned=True):
    """-> (data path, workgroup class) of one k_sh_rgb_dcrest launch; the rule of csrc/tgs_shcolor.hip written once.
    data path: None when the rest rows are not touched (levels == 1 or Mr == 0); "staged" (rows in and gradients out through LDS:
    levels^2 - 1 == Mr and tail_ok); "lds_out" (rows read directly, gradients out through LDS: levels^2 - 1 < Mr and tail_ok);
    "direct" (both directly: not tail_ok).  tail_ok: the tensor is a whole number of float4 and 16-byte aligned.
    workgroup class: "one" (P <= 256), "full" (several, all full), "ragged" (several, the last one partial)."""
    blocks = "one" if P <= PRE_BLOCK else ("full" if P % PRE_BLOCK == 0 else "ragged")
    if levels == 1 or Mr == 0:
        return None, blocks
    tail_ok = (P * Mr * 3) % 4 == 0 and aligned
    if not tail_ok:
        return "direct", blocks
    return ("staged" if levels * levels - 1 == Mr else "lds_out"), blocks


def basis(levels, dirs):
    """B[P, levels^2]: the colour's coefficient of every SH row at the direction (eval_sh on one-hot coefficients)"""
    n = levels * levels
    return eval_sh(levels - 1, torch.eye(n, dtype=dirs.dtype, device=dirs.device).unsqueeze(0), dirs)


def row_scales(sh_coordinates, sh_levels, upstream, positions=None, camera_centers=None, directions=None):
    """The per-row scales of the three comparisons, in the dtype of the inputs (float64 in the tests):
      pre      [P,3]  colour before the clamp
      color    [P,3]  0.5 + sum_k |B_k| |sh_kc|
      dsh      [P]    row norm of |B_k| |dRGB_c|, dRGB = upstream where pre >= 0 else 0
      ddir     [P]    ||A|| / max(|v|, 1e-12), A_j = sum_c |dRGB_c| sum_k |dB_k/dd_j| |sh_kc|   (|v| = 1 in direction mode)
      all_clamped [P] every channel clamped;  undecidable [P]  some |pre_c| <= 32u color_c: the kernel may clamp the other way."""
    n = sh_levels * sh_levels
    if camera_centers is not None:
        v = positions - camera_centers
        vlen = v.norm(dim=-1).clamp_min(1e-12)
        d = v / vlen[:, None]
    else:
        d, vlen = directions, torch.ones(directions.shape[0], dtype=directions.dtype, device=directions.device)
    d = d.expand(sh_coordinates.shape[0], 3)
    B = basis(sh_levels, d)
    dB = torch.stack([torch.func.jvp(lambda t: basis(sh_levels, t), (d,), (torch.eye(3, dtype=d.dtype, device=d.device)[j].expand_as(d),))[1]
                      for j in range(3)], dim=-1)                                   # [P, n, 3]
    sh = sh_coordinates[:, :n]
    pre = torch.einsum("pk,pkc->pc", B, sh) + 0.5
    color = 0.5 + torch.einsum("pk,pkc->pc", B.abs(), sh.abs())
    dRGB = torch.where(pre >= 0, upstream, torch.zeros_like(upstream))
    A = torch.einsum("pc,pkj,pkc->pj", dRGB.abs(), dB.abs(), sh.abs())
    return {"pre": pre, "color": color, "dsh": B.norm(dim=-1) * dRGB.norm(dim=-1), "ddir": A.norm(dim=-1) / vlen,
            "all_clamped": (pre < 0).all(dim=-1), "undecidable": (pre.abs() <= COLOR_U * U * color).any(dim=-1)}


def row_distances(got, want, scales, sh_levels):
    """Distances of one result from the float64 reference in units of u, each the largest over the rows of |error| / scale (the bars are
    COLOR_U, DSH_U, DDIR_U), plus the exact properties as counts of offending elements.  ``got`` / ``want``: dicts with "colors" [P,3],
    "dsh" [P,M,3] and "dvec" [P,3] (or [P,1]: positions broadcast against the camera centre) or None.  Rows flagged undecidable are left out of
    the gradient comparisons; a row whose scale is 0 must be reproduced exactly (its distance is inf otherwise)."""
    def ratio(err, scale, keep=None):
        r = torch.where(err == 0, torch.zeros_like(err), err / scale)      # x / 0 -> inf for a non-zero error on a zero scale
        if keep is not None:
            r = r[keep]
        return float(r.max() / U) if r.numel() else 0.0
    f64 = lambda t: t.detach().to(torch.float64)
    keep = ~scales["undecidable"]
    n = sh_levels * sh_levels
    P = want["colors"].shape[0]
    out = {"colors_u": ratio((f64(got["colors"]) - want["colors"]).abs(), scales["color"])}
    out["excluded_rows"] = int((~keep).sum())
    if got.get("dsh") is None:                  # colours only (a frozen group)
        return out
    dsh = f64(got["dsh"]).reshape(P, -1, 3)
    out["dsh_u"] = ratio((dsh - want["dsh"].reshape(P, -1, 3)).flatten(1).norm(dim=-1), scales["dsh"], keep)
    out["dsh_nonzero_above_levels"] = int((dsh[:, n:] != 0).sum())
    out["dsh_nonzero_clamped_rows"] = int((dsh[keep & scales["all_clamped"]] != 0).sum())
    if want.get("dvec") is not None:
        dv = f64(got["dvec"])
        if dv.shape[1] == 1:    # the sum of the three components: |sum e_j| <= sqrt(3) ||e||, and its two additions round by at most
            # 2u sum |g_j| <= 2 sqrt(3) u ||g|| with ||g|| <= ||A|| / |v| (the projection does not lengthen): sqrt(3) (128 + 2) u ||A|| / |v|
            out["dvec_u"] = ratio((dv - want["dvec"]).abs()[:, 0], scales["ddir"] * (3.0 ** 0.5 * (DDIR_U + 2.0) / DDIR_U), keep)
        else:
            out["dvec_u"] = ratio((dv - want["dvec"]).norm(dim=-1), scales["ddir"], keep)
        if sh_levels == 1:
            out["dvec_nonzero_at_one_level"] = int((dv != 0).sum())
    return out


def reference(sh_coordinates, sh_levels, upstream, positions=None, camera_centers=None, directions=None, dtype=torch.float64):
    """points_rgb and its autograd gradients in ``dtype`` -> {"colors", "dsh", "dvec"} (dvec: d positions or d directions)"""
    c = lambda t, g=False: None if t is None else t.detach().to(dtype).requires_grad_(g)
    sh, pos, dirs = c(sh_coordinates, True), c(positions, True), c(directions, True)
    col = points_rgb(sh, sh_levels, positions=pos, camera_centers=c(camera_centers), directions=dirs)
    col.backward(c(upstream))
    vec = pos if pos is not None else dirs
    return {"colors": col.detach(), "dsh": sh.grad, "dvec": vec.grad if vec.grad is not None else torch.zeros_like(vec)}
