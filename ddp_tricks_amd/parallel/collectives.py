"""Small fixed-order collectives used inside autograd ops.

``all_gather_rows`` is SyncBatchNorm's one collective per direction: every
rank contributes one short fp32 row and receives all of them in rank
order.  A gather (not an all-reduce) is used on purpose — every rank then
adds identical bytes in an identical order, so the reduced statistics are
bitwise rank-identical whatever algorithm the transport picks (the
project's fixed-order rule).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist


def _supports_gather_into_tensor(row: torch.Tensor, group) -> bool:
    backend = dist.get_backend(group)
    return row.is_cuda and backend == "nccl"


def all_gather_rows(row: torch.Tensor, group=None,
                    native: Optional[int] = None) -> torch.Tensor:
    """out[W, K] filled from each rank's row[K], on the current stream.

    Transport, in order: the native RCCL communicator the DDP wrapper
    engaged (``native`` is its handle); ``dist.all_gather_into_tensor``
    where the backend has it for the tensor's device; else a zero-padded
    ``dist.all_reduce(SUM)`` of a [W, K] buffer holding only this rank's
    row — adding fp32 zeros is exact, so the result is the same bytes."""
    row = row.contiguous()
    world = dist.get_world_size(group)
    if native is not None and row.is_cuda:
        from ..ops import load_extension
        out = torch.empty(world, row.numel(), dtype=row.dtype,
                          device=row.device)
        load_extension(required=True).rccl_all_gather(row, out, native)
        return out
    if _supports_gather_into_tensor(row, group):
        out = torch.empty(world, row.numel(), dtype=row.dtype,
                          device=row.device)
        dist.all_gather_into_tensor(out, row, group=group)
        return out
    out = torch.zeros(world, row.numel(), dtype=row.dtype, device=row.device)
    out[dist.get_rank(group)].copy_(row)
    dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
    return out
