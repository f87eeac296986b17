"""nn.Module wrappers over the framework ops.

These subclass the torch modules (identical parameter/buffer registration →
identical state_dict keys and init) but route forward through
ops/functional, which dispatches to the HIP kernels on GPU.  BN+ReLU pairs
are fused by Toy_Net using ``BatchNorm2d(..., fuse_relu=True)`` style flags
at the model level (see models/toy_net.py); the standalone modules keep
reference semantics.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import functional as F_ops


class Conv2d(nn.Conv2d):
    def forward(self, x):
        return F_ops.conv2d(x, self.weight, self.bias, self.stride, self.padding)


class Linear(nn.Linear):
    def forward(self, x):
        return F_ops.linear(x, self.weight, self.bias)


class _BatchNormBase:
    def _bn_forward(self, x, residual=None, pre_stats=None):
        self._check_input_dim(x)
        if self.training:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
        momentum = self.momentum if self.momentum is not None else 0.1
        fuse_relu = getattr(self, "fuse_relu", False)
        return F_ops.batch_norm(
            x, self.running_mean, self.running_var, self.weight, self.bias,
            self.training or not self.track_running_stats, momentum, self.eps,
            fuse_relu=fuse_relu, residual=residual, pre_stats=pre_stats)


class BatchNorm2d(nn.BatchNorm2d, _BatchNormBase):
    def __init__(self, *args, fuse_relu: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.fuse_relu = fuse_relu

    def forward(self, x, residual=None, pre_stats=None):
        # residual: optional skip tensor added before the (fused) ReLU —
        # relu(bn(x) + residual) in one kernel on GPU (ResNet blocks);
        # pre_stats: partial statistics from the producing conv's epilogue
        return self._bn_forward(x, residual, pre_stats)


class BatchNorm1d(nn.BatchNorm1d, _BatchNormBase):
    def __init__(self, *args, fuse_relu: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.fuse_relu = fuse_relu

    def forward(self, x):
        return self._bn_forward(x)


class SyncBatchNorm(nn.modules.batchnorm._BatchNorm, _BatchNormBase):
    """BatchNorm whose training statistics span every rank of
    ``process_group`` (2-D and 4-D input).

    Parameters, buffers and state_dict keys are BatchNorm1d/2d's, so
    checkpoints are interchangeable.  With world size 1, or no initialised
    process group, and in eval mode, forward IS the plain ``batch_norm``
    path: no collective, no extra kernel.  The DDP wrapper hands its
    native RCCL communicator (or none) to ``_native_comm`` so every rank
    takes the same transport."""

    is_sync_bn = True

    def __init__(self, *args, fuse_relu: bool = False, process_group=None,
                 **kwargs):
        super().__init__(*args, **kwargs)
        if not (self.affine and self.track_running_stats):
            raise ValueError("SyncBatchNorm needs affine=True and "
                             "track_running_stats=True")
        self.fuse_relu = fuse_relu
        self.process_group = process_group
        self._native_comm = None

    def _check_input_dim(self, x):
        if x.dim() not in (2, 4):
            raise ValueError(f"expected 2D or 4D input (got {x.dim()}D input)")

    def _world(self) -> int:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.process_group)

    def forward(self, x, residual=None, pre_stats=None):
        if not self.training or self._world() == 1:
            return self._bn_forward(x, residual, pre_stats)
        self._check_input_dim(x)
        if self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        momentum = self.momentum if self.momentum is not None else 0.1
        return F_ops.sync_batch_norm(
            x, self.running_mean, self.running_var, self.weight, self.bias,
            momentum, self.eps, group=self.process_group,
            native=self._native_comm, fuse_relu=self.fuse_relu,
            residual=residual, pre_stats=pre_stats)


class ReLU(nn.ReLU):
    def forward(self, x):
        return F_ops.relu(x, inplace=self.inplace)


class Dropout(nn.Dropout):
    """``nn.Dropout`` on the counter-hash mask of ``ops.dropout_rng`` (same
    mask on CPU and GPU, reproducible across a resume).  Stateless; in eval
    mode, or with a ``p`` that rounds to 0, forward returns its input object
    and launches nothing.  After a Linear + ReLU, route the junction through
    ``linear_relu_dropout`` instead so the mask rides in the GEMM epilogue."""

    def __init__(self, p: float = 0.5, inplace: bool = False):
        if inplace:
            raise ValueError("ops.modules.Dropout does not run in place")
        super().__init__(p=p, inplace=False)
        F_ops.dropout_threshold(p)      # range check

    def forward(self, x):
        return F_ops.dropout(x, self.p, self.training)


class MaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        return F_ops.max_pool2d(x, self.kernel_size, self.stride, self.padding)


class AdaptiveAvgPool2d(nn.AdaptiveAvgPool2d):
    """Only the (1,1) global case is supported (the ResNet head)."""

    def forward(self, x):
        assert self.output_size in (1, (1, 1))
        return F_ops.global_avg_pool2d(x).reshape(x.shape[0], x.shape[1], 1, 1)


class Flatten(nn.Flatten):
    """flatten(start_dim=1) with a dedicated kernel at the NHWC conv→dense
    junction: ``nn.Flatten`` on a channels_last tensor materialises the
    NCHW semantic order through ATen's strided permute-copy (~23 µs each
    way per Toy_Net step); the HIP pair does the same transpose with
    coalesced access both directions (reference utils/model.py:23)."""

    def forward(self, x):
        if (self.start_dim == 1 and self.end_dim == -1 and x.dim() == 4
                and x.is_cuda and x.dtype == torch.bfloat16
                and 1 < x.size(2) * x.size(3) <= 64 and x.size(1) > 1
                and not x.is_contiguous()  # NCHW-contig flatten is a view
                and x.is_contiguous(memory_format=torch.channels_last)
                and os.environ.get("DDPX_NHWC_FLATTEN", "1") == "1"):
            return F_ops.nhwc_flatten(x)
        return super().forward(x)


class Identity(nn.Identity):
    pass
