"""The geometry stage's renderer body, fused: ``shade`` turns ``rast`` and the vertex normals into the packed map (mask, normal, depth) in one
native forward and one native backward call, and ``render`` is the whole body of ``models/renderers/part_nvdiff_rasterizer.py`` :100-152 (and of
``ImplicitSDF.initialize_shape``, ``models/geometry/implicit_sdf.py`` :291-317) over this package: transform, ``rasterize``, vertex normals,
``shade``, ONE ``antialias`` over the packed map.

The kernels are csrc/tgs_mesh_shade.hip; the rules are written down in include/tgs_raster.h, "mesh shading".  HIP device only.  ``shade`` reads
nothing back: the camera matrix is inverted inside the kernel, the depth's extremes stay on the device.  ``render`` reads nothing back when it is
given the vertex normals or their topology (its docstring says what each omission costs).  Gradients are float32 on the device; a
backward launches nothing for an input that does not need a gradient; where ``vn`` or ``pos_clip`` is shared by the N images, the images'
gradients are added in ascending image order.  Two runs give the same bits.

Two departures from the reference's lines, both because this path never synchronises: a singular ``c2w`` makes that image's normals NaN
(``torch.linalg.inv`` raises), and an image with no covered pixel gets an all-zero depth channel (``torch.max`` of an empty tensor raises).

Not here: a gradient to ``c2w`` or ``mvp``, near-plane clipping, half precision, one fused launch for N > 1 (a loop over the images, as in the
sibling modules).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _mesh, mesh_geom, mesh_raster_grad as _dr
from ._mesh import _lib


def _rot_of(c2w: Optional[torch.Tensor]):
    """the images' c2w[:3,:3], contiguous: [N or 1, 3, 3], or None in world mode"""
    if c2w is None:
        return None
    r = c2w.detach()[..., :3, :3]
    return (r[None] if r.dim() == 2 else r).contiguous()


def _z_of(pos_clip: Optional[torch.Tensor]):
    """the clip-space z column, contiguous: [N or 1, V], or None without depth"""
    if pos_clip is None:
        return None
    z = pos_clip.detach()[..., 2]
    return (z[None] if z.dim() == 1 else z).contiguous()


def _forward(call: _mesh.Call, rast, tri, vn, camera: bool, rot, flip: bool, zattr) -> torch.Tensor:
    """the native forward of a checked call -> ``out`` [N,H,W,C]"""
    N, H, W, V, Cn, F = call[:6]
    if F == 0 or V == 0:                                                          # nothing is covered
        return torch.zeros((N, H, W, Cn), dtype=torch.float32, device=call.dev)
    out = torch.empty((N, H, W, Cn), dtype=torch.float32, device=call.dev)
    if N * H * W:
        rast_c, tri_c = rast.contiguous(), tri.contiguous()
        _mesh.run_images(_lib.tgs_meshshade, call, _mesh.shade_workspace_bytes, vn, lambda n, a: (
            V, F, tri_c.data_ptr(), a, zattr[n % len(zattr)].data_ptr() if zattr is not None else None, int(camera),
            rot[n % len(rot)].data_ptr() if rot is not None else None, int(flip), H * W, rast_c[n].data_ptr(), out[n].data_ptr()))
    return out


class _Shade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rast, tri, vn, pos_clip, c2w, camera, flip, call):
        rot, zattr = _rot_of(c2w), _z_of(pos_clip)
        out = _forward(call, rast.detach(), tri, vn.detach(), camera, rot, flip, zattr)
        ctx.call, ctx.camera, ctx.flip = call, camera, flip
        ctx.save_for_backward(rast, tri, vn, pos_clip, rot)
        return out

    @staticmethod
    def backward(ctx, g_out):
        rast, tri, vn, pos_clip, rot = ctx.saved_tensors
        need_rast, need_vn, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[2], pos_clip is not None and ctx.needs_input_grad[3]
        if not (need_rast or need_vn or need_pos):
            return (None,) * 8
        call = ctx.call
        N, H, W, V, Cn, F, dev, _ = call
        zattr = _z_of(pos_clip)
        if F == 0 or V == 0 or N * H * W == 0:                                    # nothing was covered
            return (torch.zeros_like(rast) if need_rast else None, None, torch.zeros_like(vn) if need_vn else None,
                    torch.zeros_like(pos_clip) if need_pos else None, None, None, None, None)
        d_vn = [torch.empty((V, 3), dtype=torch.float32, device=dev) for _ in range(N)] if need_vn else None
        d_z = [torch.empty((V,), dtype=torch.float32, device=dev) for _ in range(N)] if need_pos else None
        d_rast = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev) if need_rast else None
        g, rast_c, tri_c = g_out.contiguous(), rast.detach().contiguous(), tri.contiguous()
        _mesh.run_images(_lib.tgs_meshshade_backward, call, _mesh.shade_workspace_bytes, vn.detach(), lambda n, a: (
            V, F, tri_c.data_ptr(), a, zattr[n % len(zattr)].data_ptr() if zattr is not None else None, int(ctx.camera),
            rot[n % len(rot)].data_ptr() if rot is not None else None, int(ctx.flip), H * W, rast_c[n].data_ptr(), g[n].data_ptr(),
            d_vn[n].data_ptr() if need_vn else None, d_z[n].data_ptr() if need_pos else None, d_rast[n].data_ptr() if need_rast else None))
        g_vn = _mesh.input_grad(call, d_vn, vn) if need_vn else None
        g_pos = None
        if need_pos:                                                             # only the z column is non-zero
            g_pos = torch.zeros_like(pos_clip)
            g_pos[..., 2] = _mesh.input_grad(call._replace(per_image=_mesh.per_image_of(pos_clip, N)), d_z, pos_clip[..., 2])
        return d_rast, None, g_vn, g_pos, None, None, None, None


def shade(rast: torch.Tensor, tri: torch.Tensor, vn: torch.Tensor, normal_type: str = "camera", c2w: Optional[torch.Tensor] = None, flip: bool = True,
          pos_clip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rast`` [N,H,W,4] of ``rasterize``, ``tri`` [F,3] int32, ``vn`` [V,3], [1,V,3] or [N,V,3] float32 -> the packed map [N,H,W,4], or
    [N,H,W,5] when ``pos_clip`` ([V,4], [1,V,4] or [N,V,4]; its z column is read) is given.  Channel 0 is the mask (1 where a face is hit),
    channels 1..3 the normal as (n + 1) / 2, channel 4 the inverse clip z normalised to [0, 1] over the image's covered pixels; an uncovered
    pixel holds zeros.  ``normal_type`` "world": the interpolated normal, normalised, in channel order (n.y, n.z, n.x), and ``c2w`` must be
    None.  "camera": the normal through the inverse of ``c2w``'s rotation ([4,4], [3,3], [1,..] or [N,..] float32 on the device, one matrix
    per image; it never receives a gradient), turned to face the camera when ``flip``.  Differentiable with respect to ``vn``, ``pos_clip`` (z
    column) and ``rast`` (u and v).  With nothing that requires a gradient, or under ``no_grad``, it is a plain forward that saves nothing."""
    call = _mesh.shade(rast, tri, vn, normal_type, c2w, flip, pos_clip)
    camera, flip = normal_type == "camera", bool(flip)
    if not (torch.is_grad_enabled() and (rast.requires_grad or vn.requires_grad or (pos_clip is not None and pos_clip.requires_grad))):
        return _forward(call, rast.detach(), tri, vn.detach(), camera, _rot_of(c2w), flip, _z_of(pos_clip))
    return _Shade.apply(rast, tri, vn, pos_clip, c2w, camera, flip, call)


def render(glctx, verts: torch.Tensor, tri: torch.Tensor, mvp: torch.Tensor, resolution: Sequence[int], normal_type: str = "camera",
           c2w: Optional[torch.Tensor] = None, flip: bool = True, vn: Optional[torch.Tensor] = None, depth: bool = True,
           topology_hash: Optional[torch.Tensor] = None, normals_topology: Optional[mesh_geom.MeshTopology] = None,
           validate: bool = False) -> Dict[str, torch.Tensor]:
    """The renderer's body: ``verts`` [V,3], ``tri`` [F,3] int32, ``mvp`` [N,4,4], ``resolution`` (H, W) -> dict with ``opacity`` [N,H,W,1],
    ``comp_normal`` [N,H,W,3], ``comp_depth`` [N,H,W,1] (absent with ``depth=False``), ``mask`` (bool [N,H,W,1]), ``rast`` and ``pos_clip``.
    The steps: pos_clip = [verts, 1] @ mvp^T (torch); ``mesh_raster_grad.rasterize``; ``vn`` from ``mesh_geom.vertex_normals`` when not given;
    ``shade``; one ``mesh_raster_grad.antialias`` over the packed map -- the blend works per element, so every channel gets the bits a call of
    its own would give it, and the pair records are built once.  The reference's global mesh passes ``flip=False``.
    Read-backs: none with ``vn`` or ``normals_topology`` (``mesh_geom.mesh_topology(tri, V, edges=False)``, once per mesh) given; without both,
    ``vertex_normals`` builds the incidence here, one read-back per call.  ``validate=True`` adds ``rasterize``'s index check, one more; it is off
    by default, and the kernels never read through an index outside [0, V): such a face covers nothing."""
    pos_clip = torch.matmul(torch.nn.functional.pad(verts, (0, 1), value=1.0), mvp.permute(0, 2, 1)).contiguous()
    rast, _ = _dr.rasterize(glctx, pos_clip, tri, resolution, validate=validate)
    if vn is None:
        vn = mesh_geom.vertex_normals(verts, tri, normals_topology)
    packed = shade(rast, tri, vn, normal_type=normal_type, c2w=c2w, flip=flip, pos_clip=pos_clip if depth else None)
    packed = _dr.antialias(packed, rast, pos_clip, tri, topology_hash=topology_hash)
    out = {"opacity": packed[..., 0:1], "comp_normal": packed[..., 1:4], "mask": rast[..., 3:] > 0, "rast": rast, "pos_clip": pos_clip}
    if depth:
        out["comp_depth"] = packed[..., 4:5]
    return out
