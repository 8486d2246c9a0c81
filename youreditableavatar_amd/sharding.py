"""View-sharded data parallelism for the rasterizer (BASELINE.json configs 4-5): the host side.

The reference never batches (one view per optimisation step, Edit_core/tetgs_texture/refine.py:54,
257-275).  Frames are independent given the (replicated) Gaussian parameters, so a batch of V views
shards by view: each rank renders its contiguous shard view after view, autograd accumulates the
per-Gaussian gradients of every view into ONE flat fp32 buffer (parameter ``.grad`` tensors are views
into it), and the step ends with ONE all-reduce(sum) of that buffer -- RCCL over xGMI on GPUs
(backend "nccl"), gloo in the CPU tests.  There is no other data-path collective.

``FlatGradients`` and ``render_batch_sharded`` are host logic only: they run on CPU with any per-view
render function (the tests inject the CPU oracle), and nothing here touches the native library.
``multiview`` re-exports every name of this module.
"""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Sequence

import torch
import torch.distributed as dist


def shard_views(num_views: int, rank: int, world_size: int) -> range:
    """Contiguous shard of ``range(num_views)`` for ``rank``; sizes differ by at most one."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    base, extra = divmod(num_views, world_size)
    start = rank * base + min(rank, extra)
    return range(start, start + base + (1 if rank < extra else 0))


class FlatGradients:
    """One contiguous gradient buffer for a list of leaf parameters.

    ``p.grad`` of every parameter becomes a view into ``self.flat``; autograd accumulates in place
    across the views of a shard, and ``all_reduce`` sums the whole step with a single collective
    (236 B per Gaussian on the SH path = 118 MB at 500k Gaussians)."""

    PLANE_ALIGN = 64      # floats: level-major planes start on 256-byte boundaries (16-byte stores of the kernel, aligned slices for the collective)

    def __init__(self, params: Sequence[torch.Tensor], sh_params: Optional[dict] = None, level_major: bool = False):
        """``sh_params``: which parameters hold SH coefficients, NAMED by the caller -- ``{index in params: first coefficient}``: ``{4: 0}``
        for a full ``[P, 16, 3]`` tensor at position 4 (``sh_coordinates``, tetgs_model.py:268-272), ``{4: 0, 5: 1}`` for the model's
        ``_sh_coordinates_dc`` ``[P, 1, 3]`` and ``_sh_coordinates_rest`` ``[P, 15, 3]`` (:234-239).  Only these are reduced over their
        live coefficients by ``all_reduce_rows(..., sh_degree=D)``; nothing is inferred from shapes (round 6, ADVICE: a ``[P, 4, 3]``
        parameter that is not SH would have been cut to its leading rows).

        ``level_major`` (round 6): the gradients of the named SH parameters are stored coefficient by coefficient -- ``flat`` holds, per SH
        parameter, M planes of ``plane_stride`` = 3 P (rounded up to 64) floats, and ``p.grad`` is the ``[P, M, 3]`` VIEW of them with strides
        (3, plane_stride, 1).  The live coefficients of a step rendered below the stored degree are then the leading planes -- one contiguous
        slice per range of Gaussians and coefficient, handed to the collective as it is: no staging copy in front of it, none behind it
        (row-major: a strided pack and unpack of 28 MB per step at 500 k Gaussians and degree 0, 0.128 ms where no byte crosses a link).
        ``SyncFreeBatch.run_views`` sees the strides and lets the per-Gaussian pass write that layout (tgs_backward_batch_range_planes).
        An optimizer reads such a ``.grad`` like any other strided tensor."""
        self.params = list(params)
        if not self.params:
            raise ValueError("no parameters")
        self.sh_params = {int(k): int(v) for k, v in (sh_params or {}).items()}
        for i, first in self.sh_params.items():
            if not (0 <= i < len(self.params)) or self.params[i].dim() != 3 or int(self.params[i].shape[2]) != 3 or first < 0:
                raise ValueError(f"sh_params[{i}]: not a [P, M, 3] parameter of this buffer")
        dev, dt = self.params[0].device, self.params[0].dtype
        for p in self.params:
            if p.device != dev or p.dtype != dt or not p.is_leaf or not p.requires_grad:
                raise ValueError("parameters must be leaf tensors requiring grad, on one device, of one dtype")
        self.level_major = bool(level_major) and bool(self.sh_params)
        # region of parameter i in `flat`: (offset, numel, plane_stride or 0)
        self.regions, off = [], 0
        A = self.PLANE_ALIGN
        for i, p in enumerate(self.params):
            if self.level_major and i in self.sh_params:
                off = (off + A - 1) // A * A
                stride = (3 * int(p.shape[0]) + A - 1) // A * A
                n = int(p.shape[1]) * stride
                self.regions.append((off, n, stride))
            else:
                n = p.numel()
                self.regions.append((off, n, 0))
            off += n
        self.flat = torch.zeros(off, dtype=dt, device=dev)
        for p, (o, n, stride) in zip(self.params, self.regions):
            if stride:
                P, M = int(p.shape[0]), int(p.shape[1])
                p.grad = self.flat[o:o + n].view(M, stride)[:, :3 * P].view(M, P, 3).permute(1, 0, 2)     # [P, M, 3], strides (3, stride, 1)
            else:
                p.grad = self.flat[o:o + n].view_as(p)

    def zero_(self) -> None:
        self.flat.zero_()

    def all_reduce(self, group=None, async_op: bool = False, sh_degree: Optional[int] = None):
        """Sum over ranks (no-op without an initialised process group or with world size 1).  ``sh_degree``: the step's active SH degree --
        SH parameters stored for a higher one are reduced over their live coefficients only (all_reduce_rows)."""
        if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
            return None
        if sh_degree is not None and any(self._sh_live(i, sh_degree) is not None for i in range(len(self.params))):
            P = int(self.params[0].shape[0])
            if any(int(p.shape[0]) != P for p in self.params):
                raise ValueError("all_reduce(sh_degree=...) reduces by rows: every parameter must be [P, ...] with the same P")
            works = self.all_reduce_rows(0, P, group=group, sh_degree=sh_degree)
            if async_op:
                return works[0] if len(works) == 1 else _PackedReduce(works, [])
            for w in works:
                w.wait()
            return None
        return dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group, async_op=async_op)

    def row_slices(self, first: int, count: int) -> List[torch.Tensor]:
        """The pieces of ``flat`` that hold the gradients of Gaussians [first, first + count): one contiguous slice per parameter
        (every parameter is [P, ...] row-major, so a range of Gaussians is a range of rows)."""
        out = []
        for p, (off, n, stride) in zip(self.params, self.regions):
            if stride:                                       # level-major: one slice per coefficient plane
                out.extend(self.flat[off + k * stride + 3 * first: off + k * stride + 3 * (first + count)] for k in range(int(p.shape[1])))
            else:
                row = p.numel() // max(int(p.shape[0]), 1)
                out.append(self.flat[off + first * row: off + (first + count) * row])
        return out

    # ---- live SH rows ------------------------------------------------------------------------------------------------------------
    # 192 of the 236 B a Gaussian's gradients take on the SH path are dL_dsh, and the reference trains most of its iterations below the
    # stored degree: the refine stage raises `sh_levels` step by step (refine_3dgs.py:165-166), the inpainting stage stays at one level
    # (paint_2dgs.py:61-63).  Coefficients above the active degree get exactly zero gradient on every rank (backward.cu:20-139 writes
    # only the active ones), so their sum over ranks is known without moving a byte: only the (D + 1)^2 live coefficients of each SH
    # parameter are reduced -- packed into a contiguous staging slice, reduced, unpacked on wait().
    def _sh_live(self, index: int, sh_degree: Optional[int]) -> Optional[int]:
        """Live leading entries of dim 1 of parameter `index` at the active SH degree: an SH parameter whose first entry is coefficient
        `first` (``sh_params``) keeps (D + 1)^2 - first of them; None: not an SH parameter, or every entry is live.  The dead entries
        must be exactly zero on every rank (the kernels write zeros there: backward.cu:20-139 touches the active coefficients only)."""
        if sh_degree is None:
            return None
        if not self.sh_params:
            raise ValueError("sh_degree given, but this FlatGradients was built without sh_params: name the SH parameters")
        first = self.sh_params.get(index)
        if first is None:
            return None
        M = int(self.params[index].shape[1])
        live = min(max((int(sh_degree) + 1) ** 2 - first, 0), M)
        return None if live >= M else live

    def reduced_bytes(self, count: Optional[int] = None, sh_degree: Optional[int] = None) -> int:
        """Bytes per rank that all_reduce_rows(first, count, sh_degree=...) hands to the collective (count None: all Gaussians)."""
        total = 0
        for i, p in enumerate(self.params):
            P = max(int(p.shape[0]), 1)
            row = p.numel() // P
            live = self._sh_live(i, sh_degree)
            if live is not None:
                row = live * 3
            total += row * (P if count is None else int(count)) * p.element_size()
        return total

    def all_reduce_rows(self, first: int, count: int, group=None, even_alone: bool = False, sh_degree: Optional[int] = None):
        """Asynchronous sum over ranks of the gradients of Gaussians [first, first + count) -- one coalesced collective over the
        parameters' slices (a single RCCL group launch), enqueued behind whatever the current stream holds, so it runs beside the kernels
        that follow (the per-Gaussian pass over the next range, ``SyncFreeBatch.run_views(grad_chunks=..., on_chunk=...)``).  Returns the
        handles to ``wait()`` on before the gradients are used (empty without a process group).

        ``sh_degree``: the ACTIVE SH degree of the step.  SH parameters stored for a higher degree are reduced over their live
        coefficients only (see above): 44 + 12 (D + 1)^2 bytes per Gaussian instead of 236 -- 28 MB instead of 118 MB per step at 500 k
        Gaussians and degree 0.  Every rank must pass the same value.

        Coalesced or one collective per slice is decided ONCE per backend, before anything is issued and identically on every rank
        (``_coalesced_all_reduce_supported``): no exception handling around collectives that may already be in flight -- a fallback taken
        by one rank only, or after a partial issue, would double-sum or unpair them.  ``even_alone``: issue the collectives at world size 1
        too (tests: the RCCL path on a one-GPU box)."""
        if not dist.is_available() or not dist.is_initialized() or (dist.get_world_size(group) == 1 and not even_alone):
            return []
        pieces, packed = [], []
        for i, (p, (off, n, stride)) in enumerate(zip(self.params, self.regions)):
            P = max(int(p.shape[0]), 1)
            row = p.numel() // P
            live = self._sh_live(i, sh_degree)
            if stride:                                       # level-major: the live coefficients are the leading planes -- slices of `flat`, no staging
                planes = int(p.shape[1]) if live is None else live
                if count > 0 and planes > 0:
                    if first == 0 and count == P:            # all Gaussians: the planes, padding included (zeros), are ONE slice
                        pieces.append(self.flat[off: off + planes * stride])
                    else:
                        pieces.extend(self.flat[off + k * stride + 3 * first: off + k * stride + 3 * (first + count)] for k in range(planes))
            elif live is None:
                t = self.flat[off + first * row: off + (first + count) * row]
                if t.numel():
                    pieces.append(t)
            elif live > 0 and count > 0:
                src = self.flat[off + first * row: off + (first + count) * row].view(count, int(p.shape[1]), 3)[:, :live, :]
                stage = self._staging(i, first, count * live * 3)
                stage.view(count, live, 3).copy_(src)
                pieces.append(stage)
                packed.append((src, stage.view(count, live, 3)))
        if not pieces:
            return []
        if _coalesced_all_reduce_supported(group):
            with dist._coalescing_manager(group=group, async_ops=True) as cm:
                for t in pieces:
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            works = [cm]
        else:
            works = [dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True) for t in pieces]
        return [_PackedReduce(works, packed)] if packed else works

    def _staging(self, index: int, first: int, numel: int) -> torch.Tensor:
        """contiguous staging slice for the live coefficients of parameter `index`, range starting at `first` (kept from step to step;
        one per range: several ranges are in flight at once)"""
        pool = self.__dict__.setdefault("_stage", {})
        t = pool.get((index, first))
        if t is None or t.numel() != numel:
            t = pool[(index, first)] = torch.empty(numel, dtype=self.flat.dtype, device=self.flat.device)
        return t


class _PackedReduce:
    """Handle of a range whose SH parameters were reduced through staging slices: wait() waits for the collectives, then puts the summed
    live coefficients back into the flat buffer (on the current stream, behind the wait)."""

    def __init__(self, works, packed):
        self.works, self.packed = works, packed

    def wait(self):
        for w in self.works:
            w.wait()
        for dst, stage in self.packed:
            dst.copy_(stage)
        return True


_COALESCE_DECISION = {}


def _coalesced_all_reduce_supported(group=None) -> bool:
    """One group launch for several tensors (``allreduce_coalesced`` behind torch's coalescing context) exists for device tensors on the
    ``nccl`` (= RCCL) backend; gloo rejects device tensors there.  A pure function of the backend's name and of the torch build, so every
    rank decides the same; cached per backend.  ``TGS_COALESCE_ALLREDUCE=0`` forces one collective per slice (same on all ranks: the
    launcher passes the environment on)."""
    backend = str(dist.get_backend(group)).lower()
    hit = _COALESCE_DECISION.get(backend)
    if hit is None:
        hit = backend == "nccl" and hasattr(dist, "_coalescing_manager") and os.environ.get("TGS_COALESCE_ALLREDUCE", "1") != "0"
        _COALESCE_DECISION[backend] = hit
    return hit


def render_batch_sharded(render_view: Callable[[int], torch.Tensor], upstream: Callable[[int, torch.Tensor], torch.Tensor],
                         num_views: int, grads: FlatGradients, group=None, rank: Optional[int] = None,
                         world_size: Optional[int] = None, sh_degree: Optional[int] = None) -> List[int]:
    """One data-parallel step over a batch of ``num_views`` views.

    ``render_view(v)`` returns the image of view ``v`` (built on the parameters held by ``grads``);
    ``upstream(v, image)`` returns dL/d image.  After the call every rank's ``grads.flat`` holds the
    gradient of the whole batch.  Returns the views this rank rendered.  ``sh_degree``: the active SH degree the views are rendered
    with (the same on every rank) -- only the live SH coefficients are reduced (FlatGradients.all_reduce_rows)."""
    if rank is None:
        rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
    if world_size is None:
        world_size = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    mine = shard_views(num_views, rank, world_size)
    grads.zero_()
    for v in mine:
        img = render_view(v)
        img.backward(upstream(v, img.detach()))
    grads.all_reduce(group, sh_degree=sh_degree)
    return list(mine)
