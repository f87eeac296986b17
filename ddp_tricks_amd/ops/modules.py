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
        return F_ops.conv2d(x, self.weight, self.bias, self.stride,
                            self.padding, self.groups, self.dilation)


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


class GroupNorm(nn.GroupNorm):
    """``nn.GroupNorm`` (same parameters and state_dict keys) on the HIP
    GroupNorm kernels, with BatchNorm2d's fused epilogue flags so it drops
    into the same call sites: ``forward(x, residual)`` is
    relu?(gn(x) + residual).  Statistics are per (image, group): no running
    buffers, no cross-rank traffic, the same computation in train and eval."""

    is_group_norm = True

    def __init__(self, *args, fuse_relu: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.fuse_relu = fuse_relu

    def forward(self, x, residual=None, pre_stats=None):
        # pre_stats: per-channel batch partials of a conv epilogue are of no
        # use to per-image statistics; accepted for call-site parity, ignored
        return F_ops.group_norm(x, self.num_groups, self.weight, self.bias,
                                self.eps, fuse_relu=self.fuse_relu,
                                residual=residual)


class SqueezeExcite(nn.Module):
    """Squeeze-and-Excitation channel gate with the block's closing residual
    add and ReLU fused in: ``forward(u, residual, fuse_relu)`` is
    relu?(u * sigmoid(fc2(relu(fc1(mean_hw u)))) + residual).

    ``fc1`` / ``fc2`` are 1x1 convolutions in name and shape only —
    ``fc1.weight [C/r, C, 1, 1]``, ``fc2.weight [C, C/r, 1, 1]``, both with
    bias — so the state_dict keys match timm's ``se.fc1`` / ``se.fc2``; the
    junction views them as matrices for the linear kernels."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        hidden = channels // reduction
        if hidden < 1:
            raise ValueError(f"SqueezeExcite: channels {channels} // "
                             f"reduction {reduction} leaves no hidden unit")
        self.fc1 = nn.Conv2d(channels, hidden, 1)
        self.fc2 = nn.Conv2d(hidden, channels, 1)

    def forward(self, u, residual=None, fuse_relu=False):
        return F_ops.se_scale(u, self.fc1.weight, self.fc1.bias,
                              self.fc2.weight, self.fc2.bias,
                              residual=residual, fuse_relu=fuse_relu)


class LayerNorm2d(nn.Module):
    """LayerNorm over the channels of every pixel of an [N, C, H, W] tensor
    (ConvNeXt's norm): parameters ``weight`` and ``bias`` of shape [C], on the
    one-pass HIP kernels of ops/hip/ln.hip."""

    def __init__(self, channels: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))

    def forward(self, x):
        return F_ops.layer_norm2d(x, self.weight, self.bias, self.eps)


class GELU(nn.Module):
    """Exact (erf) GELU on the HIP kernel."""

    def forward(self, x):
        return F_ops.gelu(x)


class LayerScale(nn.Module):
    """``forward(u, residual)`` is residual + gamma[c] * u: ConvNeXt's
    per-channel layer scale with the block's residual add in one kernel."""

    def __init__(self, channels: int, init: float = 1e-6):
        super().__init__()
        self.gamma = nn.Parameter(torch.full((channels,), float(init)))

    def forward(self, u, residual):
        return F_ops.layer_scale(u, self.gamma, residual)


class Attention2d(nn.Module):
    """Multi-head self-attention over the H * W tokens of an [N, dim, H, W]
    activation, head dimension 64: ``qkv`` and ``proj`` are 1x1 convs on the
    MFMA implicit GEMM, so the packed qkv matrix the attention kernels of
    ops/hip/attn.hip read is the qkv conv's output as it lies."""

    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        if dim != F_ops.ATTN_HEAD_DIM * num_heads:
            raise ValueError(f"Attention2d: dim {dim} with {num_heads} heads "
                             f"is not supported; {F_ops.ATTN_SCOPE}")
        self.num_heads = num_heads
        self.qkv = Conv2d(dim, 3 * dim, 1)
        self.proj = Conv2d(dim, dim, 1)

    def forward(self, x):
        return self.proj(F_ops.attention2d(self.qkv(x), self.num_heads))


def sincos_pos_embed(dim: int, H: int, W: int, temperature: float = 10000.0):
    """Fixed 2-D sin-cos table [1, dim, H, W] of "Better plain ViT baselines":
    with omega_i = temperature^(-i / (dim/4 - 1)), i < dim/4, the channels of
    token (y, x) are [sin(x omega), cos(x omega), sin(y omega), cos(y omega)]."""
    if dim % 4 != 0 or dim < 8:
        raise ValueError(f"sincos_pos_embed: dim {dim} must be a multiple of 4,"
                         " at least 8")
    n = dim // 4
    omega = temperature ** (-torch.arange(n, dtype=torch.float64) / (n - 1))
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64),
                          torch.arange(W, dtype=torch.float64), indexing="ij")
    ax, ay = x[..., None] * omega, y[..., None] * omega       # [H, W, n]
    pe = torch.cat([ax.sin(), ax.cos(), ay.sin(), ay.cos()], dim=-1)
    return pe.permute(2, 0, 1)[None].float()


class PosEmbed2d(nn.Module):
    """Adds the fixed sin-cos table to an [N, dim, H, W] token grid.  The table
    is a non-persistent buffer built for (H, W) and rebuilt when the input's
    grid differs."""

    def __init__(self, dim: int, H: int, W: int):
        super().__init__()
        self.dim = dim
        self.register_buffer("pos", sincos_pos_embed(dim, H, W),
                             persistent=False)

    def forward(self, x):
        if x.shape[2:] != self.pos.shape[2:]:
            self.pos = sincos_pos_embed(self.dim, x.shape[2],
                                        x.shape[3]).to(self.pos.device)
        return F_ops.add_pos(x, self.pos)


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
