"""Face selections on a triangle mesh, on the device: ``refine_region`` of the painting stage (``mesh_localization.py`` :34-67) and the masks behind it.

The reference builds a pymeshlab mesh per camera, dilates and erodes the selection of the hit faces, deletes the rest, compacts, and finds the surviving
vertices again by their coordinates in a Python loop over every vertex (``mask_mesh_0822.py`` :251-252); ``gen_editing_region_mask`` (:133-148) does the same
with 8 dilations and 10 erosions and then drops the connected components smaller than a quarter of the region.  Here ``dilate_faces``, ``erode_faces``,
``refine_region``, ``face_components`` and ``keep_large_components`` take ``faces`` int32 [F,3] on the device and ``num_vertices`` and answer with masks
over the faces and the vertices of the mesh as it is: nothing is deleted, nothing is compacted, and a vertex is found by its index.

The kernels are ``csrc/tgs_mesh_region.hip``; the rules are written down in include/tgs_raster.h, "mesh regions", and restated in tests/mesh_region_ref.py.
HIP tensors only: there is no CPU path.  Everything is enqueued on the current stream.  The morphology reads nothing back; the components loop reads one
word back per ``ROUNDS_PER_READBACK`` rounds.  Integer atomics and plain stores only: two runs give the same bits.

Two differences from the reference.  It matches region vertices back to the mesh by coordinates, so a vertex that merely coincides with a region vertex is
marked too; this goes by index.  Its ``remove_duplicate_faces`` / ``remove_null_faces`` in front of the components are not done: duplicates count as faces.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch

from . import _host
from ._host import _I, _P, _Z, guard as _guard, need_device as _need_device, ok as _ok, raw_stream as _raw_stream, workspace as _workspace

SIGNATURES = {                     # name: (restype, argtypes), as include/tgs_raster.h declares them (every pointer is a c_void_p)
    "tgs_meshregion_workspace_bytes": (_Z, [_I, _I]),
    "tgs_meshregion_morph": (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _Z]),
    "tgs_meshregion_components_workspace_bytes": (_Z, [_I]),
    "tgs_meshregion_components_max_rounds": (_I, [_I]),
    "tgs_meshregion_components_begin": (_I, [_P, _I, _I, _P, _P, _P, _P, _Z]),
    "tgs_meshregion_components_rounds": (_I, [_P, _I, _P, _I, _I, _P, _P, _Z]),
    "tgs_meshregion_components_finish": (_I, [_P, _I, _P, _P, _P, _Z]),
}


def declare(lib):
    """applies ``SIGNATURES`` to a handle of the native library -> the handle"""
    return _host.declare(lib, SIGNATURES)


_lib = declare(_host.lib)
MAX_FACES = (1 << 28) - 1
MAX_ITERATIONS = 1 << 20
ROUNDS_PER_READBACK = 8            # the components loop reads its `changed` word back once per this many rounds
last_component_rounds = 0          # the rounds the last face_components call ran (its cap: tgs_meshregion_components_max_rounds(F) = F + 16)


class Region(NamedTuple):
    """``face_mask`` bool [F]: the faces that survive the reference's invert, delete and compact; ``vertex_mask`` bool [V]: the vertices some surviving face
    references, the rows of the reference's ``masked_verts``"""
    face_mask: torch.Tensor
    vertex_mask: torch.Tensor


def _mesh(faces, num_vertices) -> Tuple[int, int]:
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        got = f"{faces.dtype} {tuple(faces.shape)}" if isinstance(faces, torch.Tensor) else type(faces).__name__
        raise RuntimeError(f"expected faces as an int32 tensor of shape [F,3], got {got}")
    V, F = int(num_vertices), int(faces.shape[0])
    if V < 0:
        raise RuntimeError(f"num_vertices must be >= 0, got {V}")
    if F > MAX_FACES:
        raise RuntimeError(f"faces has {F} rows; at most 2^28 - 1 = {MAX_FACES}")
    return V, F


def _selection(name: str, sel, F: int) -> None:
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.bool or sel.dim() != 1 or sel.shape[0] != F:
        got = f"{sel.dtype} {tuple(sel.shape)}" if isinstance(sel, torch.Tensor) else type(sel).__name__
        raise RuntimeError(f"expected {name} as a bool tensor of shape [F] = [{F}], got {got}")


def _iterations(**counts) -> None:
    for name, n in counts.items():
        if not isinstance(n, int) or isinstance(n, bool) or not 0 <= n <= MAX_ITERATIONS:
            raise RuntimeError(f"{name} is an int in [0, 2^20], got {n!r}")


def _morph(sel, faces, V: int, F: int, dilate_iter: int, erode_iter: int, want_vertices: bool):
    dev = _need_device("mesh_region", faces=faces, sel=sel)
    out = torch.empty(F, dtype=torch.bool, device=dev)
    vmask = torch.empty(V, dtype=torch.bool, device=dev) if want_vertices else None
    faces_c, sel_c = faces.contiguous(), sel.contiguous()
    ws, nbytes = _workspace(_lib.tgs_meshregion_workspace_bytes(V, F), dev)
    with _guard(dev):
        _ok(_lib.tgs_meshregion_morph(_raw_stream(dev.index), V, F, faces_c.data_ptr(), sel_c.data_ptr(), dilate_iter, erode_iter, out.data_ptr(), _host.ptr(vmask),
                                      ws.data_ptr(), nbytes))
    return out, vmask


def dilate_faces(sel: torch.Tensor, faces: torch.Tensor, num_vertices: int, iterations: int = 1) -> torch.Tensor:
    """MeshLab's ``apply_selection_dilatation`` ``iterations`` times: per iteration a vertex is marked iff some incident face is selected, and a face is
    selected iff any of its three vertices is marked (the loose rule).  ``sel`` bool [F] -> bool [F].  A face with an index outside ``[0, V)`` is never
    selected and touches no vertex."""
    V, F = _mesh(faces, num_vertices)
    _selection("sel", sel, F)
    _iterations(iterations=iterations)
    return _morph(sel, faces, V, F, iterations, 0, False)[0]


def erode_faces(sel: torch.Tensor, faces: torch.Tensor, num_vertices: int, iterations: int = 1) -> torch.Tensor:
    """MeshLab's ``apply_selection_erosion`` ``iterations`` times: per iteration a vertex is marked iff it has at least one selected incident face and no
    unselected one, and a face stays selected iff all three of its vertices are marked (the strict rule).  A boundary vertex whose incident faces are all
    selected stays marked."""
    V, F = _mesh(faces, num_vertices)
    _selection("sel", sel, F)
    _iterations(iterations=iterations)
    return _morph(sel, faces, V, F, 0, iterations, False)[0]


def refine_region(faces: torch.Tensor, hit: torch.Tensor, num_vertices: int, dilate_iter: int = 1, erode_iter: int = 2) -> Region:
    """``refine_region(mesh, hit_tri_id_all_set, dilate_iter, erode_iter)`` of the reference as masks: ``hit`` is a bool [F], which is what ``hit_faces``
    returns, or an integer index tensor; the hit faces are selected, dilated ``dilate_iter`` times, eroded ``erode_iter`` times.  An empty ``hit`` gives empty
    masks.  The defaults (1, 2) are the reference's; it uses (2, 5) for the first eight cameras and (8, 10) for the localisation."""
    V, F = _mesh(faces, num_vertices)
    if isinstance(hit, torch.Tensor) and hit.dtype in (torch.int32, torch.int64) and hit.dim() == 1:
        dev = _need_device("mesh_region", faces=faces, hit=hit)
        idx = hit.long()
        sel = torch.zeros(F + 1, dtype=torch.bool, device=dev)
        sel[torch.where((idx >= 0) & (idx < F), idx, F)] = True                 # an index outside [0, F) selects nothing (it lands on the spare row: no read-back)
        sel = sel[:F]
    else:
        _selection("hit", hit, F)
        sel = hit
    _iterations(dilate_iter=dilate_iter, erode_iter=erode_iter)
    return Region(*_morph(sel, faces, V, F, dilate_iter, erode_iter, True))


def face_components(face_mask: torch.Tensor, faces: torch.Tensor, num_vertices: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The connected components of the selected faces -> (``label`` int32 [F], ``size`` int32 [F]).  Two selected faces are adjacent iff they share an
    undirected edge, the same unordered pair of distinct vertex indices; faces around a non-manifold edge are all adjacent; sharing only a vertex does not
    connect.  ``label`` is the smallest face index of the component and ``size`` its face count; unselected faces get -1 and 0.  Reads one word back per
    ``ROUNDS_PER_READBACK`` rounds; the loop ends at the library's cap of F + 16 rounds with an error and never spins."""
    global last_component_rounds
    V, F = _mesh(faces, num_vertices)
    _selection("face_mask", face_mask, F)
    dev = _need_device("mesh_region", faces=faces, face_mask=face_mask)
    label, size = torch.empty(F, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
    last_component_rounds = 0
    if F == 0:
        return label, size
    faces_c, sel_c = faces.contiguous(), face_mask.contiguous()
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_lib.tgs_meshregion_components_workspace_bytes(F), dev)
    with _guard(dev):
        stream = _raw_stream(dev.index)
        _ok(_lib.tgs_meshregion_components_begin(stream, V, F, faces_c.data_ptr(), sel_c.data_ptr(), label.data_ptr(), ws.data_ptr(), nbytes))
        done = 0
        while True:
            _ok(_lib.tgs_meshregion_components_rounds(stream, F, label.data_ptr(), done, ROUNDS_PER_READBACK, changed.data_ptr(), ws.data_ptr(), nbytes))     # at the cap: an error
            done += ROUNDS_PER_READBACK
            if int(changed.item()) == 0:                                        # the read-back
                break
        _ok(_lib.tgs_meshregion_components_finish(stream, F, label.data_ptr(), size.data_ptr(), ws.data_ptr(), nbytes))
    last_component_rounds = done
    return label, size


def keep_large_components(face_mask: torch.Tensor, faces: torch.Tensor, num_vertices: int, min_faces: int) -> torch.Tensor:
    """``meshing_remove_connected_component_by_face_number(mincomponentsize=min_faces)`` as a mask: a selected face is kept iff its component has
    ``size >= min_faces`` faces (the reference deletes the components strictly smaller).  Duplicate faces count as faces."""
    label, size = face_components(face_mask, faces, num_vertices)
    return (label >= 0) & (size >= int(min_faces))
