"""Autograd-integrated ops: HIP/CDNA4 kernels on GPU, torch reference on CPU.

GPU data layout: activations are bf16 **channels_last** (NHWC — channels
fastest, the MFMA implicit-GEMM-friendly layout on CDNA4); weights are
cached per-parameter-version as bf16 channels_last (KRSC) plus the
transformed WT2[C, R·S·K] operand for backward-data.  Statistics, biases,
losses and weight gradients are fp32 (the framework's amp-O1 policy —
reference behavior via apex at utils/train.py:58).

On CPU (the no-GPU test tier) the same entry points run equivalent torch
ops in fp32, doubling as the numerics oracle the GPU tests compare against.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import require_ext_for
from .. import amp as amp_mod

CL = torch.channels_last


# --------------------------------------------------------------- casting ---

_WCACHE = {}  # param -> {"version": v, variant: tensor}


def weight_variant(w: torch.Tensor, variant: str) -> torch.Tensor:
    """Per-step cached transforms of fp32 master weights.

    variants: "flat"     — bf16, native contiguous (linear [N,K])
              "nhwc"     — bf16 channels_last (conv KRSC memory)
              "wt2"      — bf16 [C, R*S*K] (conv dgrad operand)
              "nhwc_p8"  — bf16 channels_last with Cin zero-padded to 8
                           (MFMA path for C<8 stems, e.g. ResNet RGB)
              "wt2_p8"   — dgrad operand of the padded weights

    An entry is valid while ``w._version`` is unchanged, so every in-place
    write to the parameter itself (``w.mul_()``, ``w.copy_()``,
    ``load_state_dict``, a torch optimizer step) invalidates it.  Writes
    through ``w.data`` (or ``w.detach()``, or a kernel handed the raw
    storage) are INVISIBLE here: ``w.data`` carries its own version counter
    and ``w.data = t`` keeps the old one.  Whoever writes that way must call
    ``clear_weight_cache()`` afterwards (FusedSGD, Lookahead and the DDP
    parameter broadcast do).
    """
    ent = _WCACHE.get(w)
    if ent is None or ent["version"] != w._version:
        ent = {"version": w._version}
        _WCACHE[w] = ent
    if variant not in ent:
        ext = require_ext_for(w) if w.is_cuda else None
        if (ext is not None and w.dtype == torch.float32
                and variant in ("nhwc", "wt2", "nhwc_p8", "wt2_p8")):
            # one fused kernel fills BOTH conv operand layouts per step
            pad8 = variant.endswith("_p8")
            sfx = "_p8" if pad8 else ""
            nhwc, wt2 = ext.pack_conv_weight(w.detach().contiguous(), pad8,
                                             True)
            ent["nhwc" + sfx] = nhwc
            ent["wt2" + sfx] = wt2
            return ent[variant]
        wb = w.detach().to(torch.bfloat16)
        if variant == "flat":
            ent[variant] = wb.contiguous()
        elif variant == "nhwc":
            ent[variant] = wb.contiguous(memory_format=CL)
        elif variant == "wt2":
            K, C, R, S = w.shape
            ent[variant] = wb.permute(1, 2, 3, 0).reshape(C, R * S * K).contiguous()
        elif variant in ("nhwc_p8", "wt2_p8"):
            K, C, R, S = w.shape
            wp = torch.zeros(K, 8, R, S, dtype=torch.bfloat16, device=w.device)
            wp[:, :C] = wb
            if variant == "nhwc_p8":
                ent[variant] = wp.contiguous(memory_format=CL)
            else:
                ent[variant] = wp.permute(1, 2, 3, 0).reshape(8, R * S * K).contiguous()
        else:
            raise KeyError(variant)
    return ent[variant]


def clear_weight_cache() -> None:
    _WCACHE.clear()


# ------------------------------------------------------- skip-grad fusion ---

def _skipfuse_on() -> bool:
    """ResNet skip-gradient fusion: at a residual
    junction the block input is consumed twice — by the first conv and as
    the BN epilogue's residual — so autograd sums conv-dgrad dx with the
    BN's dresid in a separate ATen add pass (4.3% of the ResNet-50 step).
    With fusion on, the BN stashes dresid in a box attached to the shared
    tensor object and returns None; the conv's dgrad (which runs strictly
    later — it is upstream in the backward order) streams it into its
    epilogue (dx += dresid in-flight)."""
    return os.environ.get("DDPX_SKIPFUSE", "1") == "1"


def _attach_skipbox(ctx, x):
    """Conv-side: ensure the input tensor carries a junction box and
    remember it on the ctx (object attribute — allocator-reuse immune)."""
    box = getattr(x, "_ddpx_skipbox", None)
    if box is None:
        box = {}
        x._ddpx_skipbox = box
    ctx.skip_box = box


def _pop_skip_grad(ctx):
    box = getattr(ctx, "skip_box", None)
    if box is None:
        return None
    return box.pop("g", None)


def bf16_weight(w: torch.Tensor) -> torch.Tensor:
    if w.dtype == torch.bfloat16:
        return w
    return weight_variant(w, "flat")


def _to_bf16(x: torch.Tensor) -> torch.Tensor:
    return x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)


def _chlast(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 4:
        return x.contiguous(memory_format=CL)
    return x.contiguous()


def _nhwc_2d(x: torch.Tensor) -> torch.Tensor:
    """Zero-copy [N*H*W, C] view of a channels_last 4D tensor."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


# ----------------------------------------------------------------- conv2d ---

def _pad8(xb: torch.Tensor) -> torch.Tensor:
    """Zero-pad channels to 8 (channels_last) so C<8 inputs can take the
    MFMA implicit-GEMM path — one fused kernel on GPU."""
    ext = require_ext_for(xb)
    if ext is not None:
        return ext.pad8_channels(xb)
    N, C, H, W = xb.shape
    xp = torch.zeros(N, 8, H, W, dtype=xb.dtype, device=xb.device)
    xp = xp.contiguous(memory_format=CL)
    xp[:, :C] = xb
    return xp


def _use_pad8(C: int, H: int, W: int) -> bool:
    return C < 8 and H * W >= 1024


def _conv_fwd_prep(ctx, x, weight, bias, stride, padding):
    """Shared operand prep for the conv autograd functions; returns
    (ext, xb_for_kernel, wb, bias_f) and fills ctx bookkeeping."""
    ext = require_ext_for(x)
    xb = _chlast(_to_bf16(x))
    C_in = weight.shape[1]
    if C_in < 8:
        pad8_bwd = _use_pad8(C_in, xb.shape[2], xb.shape[3])
        xp = _pad8(xb)
        wb = weight_variant(weight, "nhwc_p8")
        ctx.save_for_backward(xp if pad8_bwd else xb, weight)
        ctx.meta = (stride, padding, x.dtype, weight.shape,
                    bias is not None, pad8_bwd)
        return ext, xp, wb, (bias if bias is None else bias.detach().float())
    wb = weight_variant(weight, "nhwc")
    ctx.save_for_backward(xb, weight)
    ctx.meta = (stride, padding, x.dtype, weight.shape, bias is not None,
                False)
    if stride == 1 and x.is_cuda and _skipfuse_on():
        _attach_skipbox(ctx, x)
    if stride == 1 and xb is x \
            and os.environ.get("DDPX_BNFUSE", "0") == "1":
        # producer-side BN-backward fusion (attr set by batch_norm).
        # OPT-IN: measured net-negative at ResNet-50 (8.38k vs 8.72k
        # img/s) — the epilogue's +32 VGPR (partial accumulators +
        # coefficient cache) pushes the dgrad to the 512-reg cliff while
        # the skipped BN partial pass only saves ~1 activation read.
        ctx.bn_box = getattr(x, "_ddpx_bnbwd", None)
    return ext, xb, wb, (bias if bias is None else bias.detach().float())


def _conv_bwd_impl(ctx, dy):
    xb, weight = ctx.saved_tensors
    stride, padding, x_dtype, w_shape, has_bias, pad8 = ctx.meta
    ext = require_ext_for(dy)
    dyb = _chlast(_to_bf16(dy))
    K, C, R, S = w_shape
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        # the dgrad kernel writes 8-channel chunks: a C<8 conv whose
        # UNPADDED x was saved (small spatial) still takes the padded
        # operand, and the pad channels are sliced off below
        p8 = pad8 or C < 8
        wt2 = weight_variant(weight, "wt2_p8" if p8 else "wt2")
        box = getattr(ctx, "bn_box", None)
        # stashed junction skip-grad (only ever set for stride-1 non-pad8
        # convs — see _attach_skipbox call sites)
        g = _pop_skip_grad(ctx) if (stride == 1 and not pad8) else None
        if (box is not None and not pad8 and stride == 1
                and x_dtype != torch.float32 and g is None):
            dx, slab = ext.conv2d_dgrad_bn(
                dyb, wt2, xb.shape[0], xb.shape[1], xb.shape[2], xb.shape[3],
                R, S, padding, box["x"], box["mask"], box["mean"],
                box["invstd"])
            box["slab"] = slab
            box["dx_ref"] = dx
        else:
            dx = ext.conv2d_dgrad(dyb, wt2, xb.shape[0],
                                  8 if p8 else xb.shape[1],
                                  xb.shape[2], xb.shape[3], R, S,
                                  stride, padding, g)
            if p8:
                dx = dx[:, :C]
            if x_dtype == torch.float32:
                dx = dx.float()
    want_db = has_bias and ctx.needs_input_grad[2]
    # the wgrad kernels already hold every dy element: with both grads
    # wanted the bias sums ride along instead of re-reading dy
    # (DDPX_WGRAD_BIAS=0 restores the separate col_sum pass)
    fuse_db = (want_db and ctx.needs_input_grad[1]
               and os.environ.get("DDPX_WGRAD_BIAS", "1") != "0")
    if ctx.needs_input_grad[1]:
        if fuse_db:
            dw, db = ext.conv2d_wgrad_bias(dyb, xb, R, S, stride, padding)
        else:
            dw = ext.conv2d_wgrad(dyb, xb, R, S, stride, padding)
        if pad8:
            dw = dw[:, :C].contiguous()
    if want_db and not fuse_db:
        db = ext.col_sum(_nhwc_2d(dyb))
    return dx, dw, db


class _HIPConv2dStats(torch.autograd.Function):
    """Conv forward that also emits the consuming BN's partial statistics
    from the epilogue (stats output is non-differentiable)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding):
        ext, xk, wb, bias_f = _conv_fwd_prep(ctx, x, weight, bias, stride,
                                             padding)
        y, stats = ext.conv2d_fwd_stats(xk, wb, bias_f, stride, padding)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, dstats):
        dx, dw, db = _conv_bwd_impl(ctx, dy)
        return dx, dw, db, None, None


class _HIPConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        C_in = weight.shape[1]
        if C_in < 8:
            # fwd always takes the MFMA path on zero-padded channels
            # (measured faster than the direct VALU kernel even at MNIST
            # size: 48 vs 64 us).  wgrad for SMALL spatial inputs stays on
            # the specialized C<8 kernels (measured: MFMA wgrad at Kgemm=72
            # is 362 us vs 132 us for the sliding-window kernel), so the
            # UNPADDED x is saved in that case.
            pad8_bwd = _use_pad8(C_in, xb.shape[2], xb.shape[3])
            xp = _pad8(xb)
            wb = weight_variant(weight, "nhwc_p8")
            y = ext.conv2d_fwd(xp, wb, bias if bias is None
                               else bias.detach().float(), stride, padding)
            ctx.save_for_backward(xp if pad8_bwd else xb, weight)
            ctx.meta = (stride, padding, x.dtype, weight.shape,
                        bias is not None, pad8_bwd)
            return y
        wb = weight_variant(weight, "nhwc")
        bias_f = bias if bias is None else bias.detach().float()
        y = ext.conv2d_fwd(xb, wb, bias_f, stride, padding)
        ctx.save_for_backward(xb, weight)
        ctx.meta = (stride, padding, x.dtype, weight.shape, bias is not None,
                    False)
        if stride == 1 and x.is_cuda and _skipfuse_on():
            _attach_skipbox(ctx, x)
        if stride == 1 and xb is x \
                and os.environ.get("DDPX_BNFUSE", "0") == "1":
            # producer-side BN-backward fusion (opt-in; see _conv_fwd_prep)
            ctx.bn_box = getattr(x, "_ddpx_bnbwd", None)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db = _conv_bwd_impl(ctx, dy)
        return dx, dw, db, None, None


def _uniform(v, name):
    """The HIP conv kernels take ONE stride and ONE padding for both
    spatial dims: reduce a uniform tuple to its value, refuse any other."""
    if isinstance(v, (tuple, list)):
        if any(e != v[0] for e in v):
            raise ValueError(
                f"HIP conv2d needs a uniform {name}, got {tuple(v)}")
        return v[0]
    return v


def conv2d(x, weight, bias=None, stride=1, padding=0):
    if x.is_cuda and require_ext_for(x) is not None:
        stride = _uniform(stride, "stride")
        padding = _uniform(padding, "padding")
        # NOTE: a 1x1-as-GEMM route through the linear kernels was tried and
        # REVERTED — measured 2.6 ms vs 0.27 ms for the conv path at
        # ResNet-50's [M~800k, 64x64] shapes (the GEMM ladder's split-K is
        # tuned for classifier-head sizes, the conv wgrad splits for deep M).
        return _HIPConv2d.apply(x, weight, bias, stride, padding)
    if x.is_cuda and amp_mod.is_enabled():  # explicit torch-fallback bring-up path
        return F.conv2d(_to_bf16(x), bf16_weight(weight).view_as(weight),
                        bias.to(torch.bfloat16) if bias is not None else None,
                        stride, padding)
    return F.conv2d(x, weight, bias, stride, padding)


# ----------------------------------------------------------------- linear ---

class _HIPLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ext = require_ext_for(x)
        xb = _to_bf16(x.contiguous())
        wb = weight_variant(weight, "flat")
        bias_f = bias if bias is None else bias.detach().float()
        y = ext.linear_fwd(xb, wb, bias_f)
        ctx.save_for_backward(xb, wb)
        ctx.meta = (x.dtype, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        x_dtype, has_bias = ctx.meta
        ext = require_ext_for(dy)
        dyb = _to_bf16(dy.contiguous())
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ext.linear_dgrad(dyb, wb)
            if x_dtype == torch.float32:
                dx = dx.float()
        if ctx.needs_input_grad[1]:
            dw = ext.linear_wgrad(dyb, xb)
        if has_bias and ctx.needs_input_grad[2]:
            db = ext.col_sum(dyb)
        return dx, dw, db


def linear(x, weight, bias=None):
    if x.is_cuda and require_ext_for(x) is not None:
        return _HIPLinear.apply(x, weight, bias)
    if x.is_cuda and amp_mod.is_enabled():
        return F.linear(_to_bf16(x), bf16_weight(weight),
                        bias.to(torch.bfloat16) if bias is not None else None)
    return F.linear(x, weight, bias)


# ---------------------------------------------------------------- dropout ---
#
# Counter-hash dropout: the mask is a pure function of (seed, rank, epoch,
# call number, element offset) — layout in ops/hip/common.h — so it is the
# same on CPU and GPU, needs no stored mask tensor and is reproduced by a
# resumed run (the call counter restarts with every epoch).

_U64 = (1 << 64) - 1
# seed salts of the dropout stream (ops/hip/common.h, dropout header)
DROP_SALT = 0xA0761D6478BD642F
DROP_RANK_SALT = 0xE7037ED1A0B428DB


def _drop_hash(s: int, key: int) -> int:
    """``h(s, key)`` of the kernels, in Python integers modulo 2^64."""
    z = (s + (key + 1) * 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def dropout_threshold(p: float) -> int:
    """Drop probability as the kernels' 16-bit threshold
    ``floor(p*65536 + 0.5)``: an element is dropped when its 16 hashed bits
    are below it, so the effective probability is ``thr/65536``.  ``p < 0``
    and a ``p`` that rounds to 65536 (everything dropped) are refused."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    thr = int(math.floor(p * 65536.0 + 0.5))
    if thr > 65535:
        raise ValueError(
            f"dropout probability {p} rounds to 1 (threshold {thr} > 65535)")
    return thr


def dropout_scale(thr: int) -> float:
    """``float32(65536 / (65536 - thr))``, the kept elements' factor (exactly
    1 for ``thr == 0``)."""
    return float(np.float32(65536.0 / (65536.0 - thr)))


def dropout_mask(call_seed: int, numel: int, thr: int) -> np.ndarray:
    """The numpy mirror of the kernels' mask: bool [numel], True where
    element ``i`` (offset in the output's dense storage) is KEPT."""
    u = np.uint64
    i = np.arange(int(numel), dtype=np.uint64)
    s = np.full(1, int(call_seed) & _U64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = s + ((i >> u(2)) + u(1)) * u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    lane = (z >> (u(16) * (i & u(3)))) & u(0xFFFF)
    return lane >= u(int(thr))


class DropoutRNG:
    """Host side of the dropout stream: hands one 64-bit ``call_seed`` to
    every dropout call in training,

        call_seed = h(seed ^ DROP_SALT ^ rank*DROP_RANK_SALT,
                      (epoch << 32) | calls)

    in Python integers — no tensor, no H2D copy, no sync.  ``set_epoch``
    restarts the call counter, so a run resumed at an epoch boundary draws
    the masks the uninterrupted run would have."""

    def __init__(self):
        self._seed = 0
        self.rank = 0
        self.epoch = 0
        self.calls = 0

    def seed(self, seed: int, rank=None) -> None:
        """Key the stream; ``rank`` defaults to the initialised process
        group's rank, else 0.  Restarts epoch 0, call 0."""
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if (dist.is_available()
                                       and dist.is_initialized()) else 0
        self._seed = int(seed) & _U64
        self.rank = int(rank)
        self.epoch = 0
        self.calls = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        self.calls = 0

    def next_call_seed(self) -> int:
        base = (self._seed ^ DROP_SALT
                ^ (self.rank * DROP_RANK_SALT)) & _U64
        key = ((self.epoch << 32) | (self.calls & 0xFFFFFFFF)) & _U64
        self.calls += 1
        return _drop_hash(base, key)

    def state_dict(self) -> dict:
        return {"seed": self._seed, "rank": self.rank, "epoch": self.epoch,
                "calls": self.calls}

    def load_state_dict(self, sd: dict) -> None:
        self._seed = int(sd["seed"]) & _U64
        self.rank = int(sd["rank"])
        self.epoch = int(sd["epoch"])
        self.calls = int(sd["calls"])


dropout_rng = DropoutRNG()


def _seed_i64(call_seed: int) -> int:
    """The bindings take the 64 seed bits as int64."""
    return call_seed - (1 << 64) if call_seed >> 63 else call_seed


def _storage_mask(call_seed: int, thr: int, like: torch.Tensor):
    """``dropout_mask`` laid out over ``like`` (a dense contiguous or
    channels_last tensor), indexed in storage order."""
    m = torch.from_numpy(dropout_mask(call_seed, like.numel(), thr))
    m = m.to(like.device)
    if like.is_contiguous():
        return m.view(like.shape)
    N, C, H, W = like.shape
    return m.view(N, H, W, C).permute(0, 3, 1, 2)


def _dense(x: torch.Tensor) -> torch.Tensor:
    if x.is_contiguous() or (x.dim() == 4
                             and x.is_contiguous(memory_format=CL)):
        return x
    return x.contiguous()


def _torch_drop(v: torch.Tensor, call_seed: int, thr: int) -> torch.Tensor:
    """The kernels' formula in torch: v*scale (rounded to v's dtype) where
    kept, +0 where dropped."""
    scale = dropout_scale(thr)
    keep = _storage_mask(call_seed, thr, v)
    scaled = (v.float() * scale).to(v.dtype) if v.dtype != torch.float64 \
        else v * scale
    return torch.where(keep, scaled, torch.zeros_like(scaled))


class _HIPDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, thr, scale, call_seed):
        ext = require_ext_for(x)
        xd = _dense(x)
        ctx.meta = (thr, scale, call_seed, not xd.is_contiguous())
        return ext.dropout_fwd(xd, thr, scale, call_seed)

    @staticmethod
    def backward(ctx, dy):
        thr, scale, call_seed, chlast = ctx.meta
        ext = require_ext_for(dy)
        # dy takes the forward's layout: the mask is indexed by storage offset
        dy = dy.contiguous(memory_format=CL) if chlast else dy.contiguous()
        return ext.dropout_bwd(dy, thr, scale, call_seed), None, None, None


def dropout(x, p: float = 0.5, training: bool = True):
    """Counter-hash dropout.  In eval mode, or when ``p`` rounds to a zero
    threshold, returns ``x`` itself with no launch and no draw from
    ``dropout_rng``."""
    thr = dropout_threshold(p) if training else 0
    if thr == 0:
        return x
    call_seed = dropout_rng.next_call_seed()
    if x.is_cuda and require_ext_for(x) is not None:
        if x.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"HIP dropout takes bf16 or fp32, got {x.dtype}")
        return _HIPDropout.apply(x, thr, dropout_scale(thr),
                                 _seed_i64(call_seed))
    return _torch_drop(_dense(x), call_seed, thr)


class _HIPLinearAct(torch.autograd.Function):
    """dropout(relu(linear(x))) with the ReLU and the mask in the GEMM
    epilogue.  Saves xb, wb and the output y; the backward reads the mask
    off y (y > 0 iff kept and active, as scale >= 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias, thr, scale, call_seed):
        ext = require_ext_for(x)
        xb = _to_bf16(x.contiguous())
        wb = weight_variant(weight, "flat")
        bias_f = bias if bias is None else bias.detach().float()
        y = ext.linear_act_fwd(xb, wb, bias_f, thr, scale, call_seed)
        ctx.save_for_backward(xb, wb, y)
        ctx.meta = (x.dtype, bias is not None, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, wb, y = ctx.saved_tensors
        x_dtype, has_bias, scale = ctx.meta
        ext = require_ext_for(dy)
        dz = ext.relu_drop_bwd(_to_bf16(dy.contiguous()), y, scale)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ext.linear_dgrad(dz, wb)
            if x_dtype == torch.float32:
                dx = dx.float()
        if ctx.needs_input_grad[1]:
            dw = ext.linear_wgrad(dz, xb)
        if has_bias and ctx.needs_input_grad[2]:
            db = ext.col_sum(dz)
        return dx, dw, db, None, None, None


def linear_relu_dropout(lin_mod, drop_mod, x):
    """The Linear -> ReLU -> Dropout junction as one op.  GPU: one GEMM
    with the fused epilogue (training: ReLU + dropout; eval or ``p`` that
    rounds to 0: ReLU alone, no draw from ``dropout_rng``).  CPU: the same
    formula in torch with the mirror's mask, so a CPU model and a GPU model
    draw identical masks."""
    thr = dropout_threshold(drop_mod.p) if drop_mod.training else 0
    call_seed = dropout_rng.next_call_seed() if thr else 0
    if x.is_cuda and require_ext_for(x) is not None:
        return _HIPLinearAct.apply(x, lin_mod.weight, lin_mod.bias, thr,
                                   dropout_scale(thr), _seed_i64(call_seed))
    y = torch.relu(linear(x, lin_mod.weight, lin_mod.bias))
    if thr == 0:
        return y
    return _torch_drop(y.contiguous(), call_seed, thr)


# ------------------------------------------------------------- batch norm ---

class _HIPBatchNorm(torch.autograd.Function):
    """BatchNorm (2d channels_last or 1d) with optional fused ReLU.

    fp32 stats over bf16 activations; running stats updated in-place
    (rank-local; broadcast from rank 0 each forward by the DDP wrapper —
    reference broadcast_buffers semantics)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                training, momentum, eps, fuse_relu, residual, pre_stats=None):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        rb = None if residual is None else _chlast(_to_bf16(residual))
        if training:
            y, save_mean, save_invstd, mask = ext.bn_fwd_train(
                xb, weight.detach(), bias.detach(), running_mean, running_var,
                momentum, eps, fuse_relu, rb, pre_stats)
            ctx.save_for_backward(xb, weight, save_mean, save_invstd, mask)
            # producer-side bwd fusion: the conv that consumes y can emit
            # this BN's backward partials from its dgrad epilogue; the box
            # carries what it needs and brings the result back (used only
            # when dy's identity proves a single consumer — see backward)
            ctx.bnbwd_box = {"x": xb, "mask": mask, "mean": save_mean,
                             "invstd": save_invstd, "slab": None,
                             "dx_ref": None}
        elif (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
              or ctx.needs_input_grad[2]):
            # (grad mode is force-disabled inside Function.forward, so the
            # needs_input_grad flags — not torch.is_grad_enabled() — tell
            # whether a backward will run)
            # eval-mode BN on the grad path (fine-tuning with frozen stats;
            # VERDICT r01 weak #8): keep the relu mask + frozen stats for
            # backward.  The C-length stat vectors are cloned — the DDP
            # buffer broadcast rewrites the originals in place each forward.
            y, mask = ext.bn_fwd_eval_mask(xb, weight.detach(), bias.detach(),
                                           running_mean, running_var, eps,
                                           fuse_relu, rb)
            ctx.save_for_backward(xb, weight, running_mean.detach().clone(),
                                  running_var.detach().clone(), mask)
            ctx.eps = eps
        else:
            y = ext.bn_fwd_eval(xb, weight.detach(), bias.detach(),
                                running_mean, running_var, eps, fuse_relu, rb)
        ctx.fuse_relu = fuse_relu
        ctx.training = training
        ctx.x_dtype = x.dtype
        ctx.has_residual = residual is not None
        # skip-grad fusion arming: the residual tensor is ALSO the junction
        # conv's input (its box was attached by that conv's forward, which
        # ran earlier).  Stash dresid there in backward instead of
        # returning it; the conv's dgrad (strictly later in backward
        # order) streams it into its epilogue.
        ctx.skip_armed = False
        if (training and residual is not None and residual.is_cuda
                and residual.dtype == torch.bfloat16 and _skipfuse_on()
                and residual.requires_grad):
            sb = getattr(residual, "_ddpx_skipbox", None)
            if sb is not None:
                ctx.skip_armed = True
                ctx.skip_stash = sb
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            # frozen-stats backward: mean/var are constants, so
            # dx = gamma*invstd*dy_eff (eval_stats=True zeroes the batch
            # correction terms); dgamma/dbeta reduce against frozen xhat
            xb, weight, rm, rv, mask = ctx.saved_tensors
            ext = require_ext_for(dy)
            dyb = _chlast(_to_bf16(dy))
            si = (rv + ctx.eps).rsqrt()
            out = ext.bn_bwd(xb, dyb, weight.detach(), rm, si, mask,
                             ctx.fuse_relu, ctx.has_residual, None, True)
            dx, dweight, dbias = out[0], out[1], out[2]
            dresid = out[3] if ctx.has_residual else None
            if ctx.x_dtype == torch.float32:
                dx = dx.float()
            return (dx, dweight, dbias, None, None, None, None, None, None,
                    dresid, None)
        xb, weight, save_mean, save_invstd, mask = ctx.saved_tensors
        ext = require_ext_for(dy)
        box = getattr(ctx, "bnbwd_box", None)
        pre_slab = None
        if (box is not None and box["slab"] is not None
                and dy is box["dx_ref"]):
            # dy IS the consuming conv's dgrad output (single consumer —
            # a multi-consumer sum would be a different tensor object), so
            # the partials it emitted are exactly this BN's
            pre_slab = box["slab"]
        dyb = _chlast(_to_bf16(dy))
        out = ext.bn_bwd(xb, dyb, weight.detach(), save_mean,
                         save_invstd, mask, ctx.fuse_relu, ctx.has_residual,
                         pre_slab)
        dx, dweight, dbias = out[0], out[1], out[2]
        dresid = out[3] if ctx.has_residual else None
        if ctx.x_dtype == torch.float32:
            dx = dx.float()
        if dresid is not None and getattr(ctx, "skip_armed", False):
            stash = ctx.skip_stash
            prev = stash.get("g")
            stash["g"] = dresid if prev is None else prev + dresid
            dresid = None   # delivered through the junction conv's dgrad
        return (dx, dweight, dbias, None, None, None, None, None, None,
                dresid, None)


def batch_norm(x, running_mean, running_var, weight, bias,
               training, momentum, eps, fuse_relu=False, residual=None,
               pre_stats=None):
    """BN with optionally fused ReLU and residual add: relu(bn(x) + residual)
    — the ResNet block epilogue in one kernel (skip grad returned in bwd).
    pre_stats: [2,C,S] partial sums emitted by the producing conv's epilogue
    (conv2d_stats) — skips the BN statistics pass entirely."""
    if x.is_cuda and require_ext_for(x) is not None:
        y = _HIPBatchNorm.apply(x, weight, bias, running_mean, running_var,
                                training, momentum, eps, fuse_relu,
                                residual, pre_stats)
        # surface the producer-fusion box on the tensor object so the
        # consuming conv can find it (object-attribute, not data_ptr —
        # immune to allocator reuse); ctx attributes are visible on grad_fn
        if training and y.grad_fn is not None:
            box = getattr(y.grad_fn, "bnbwd_box", None)
            if box is not None:
                y._ddpx_bnbwd = box
        return y
    xf = x.float() if x.dtype != torch.float32 else x
    y = F.batch_norm(xf, running_mean, running_var, weight, bias,
                     training, momentum, eps)
    if residual is not None:
        y = y + residual.float()
    if fuse_relu:
        y = F.relu(y)
    return y.to(x.dtype) if x.is_cuda and amp_mod.is_enabled() else y


# -------------------------------------------------------- sync batch norm ---

def _gather_rows(row, group, native):
    from ..parallel.collectives import all_gather_rows
    return all_gather_rows(row, group, native)


class _HIPSyncBatchNorm(torch.autograd.Function):
    """Training BatchNorm over the batch of every rank in ``group``.

    Forward: local partial sums -> one gathered [W, 2C+2] row set ->
    finalize + apply.  Backward: local dbeta/dgamma sums -> one gathered
    [W, 2C] row set -> coefficients + dx.  The memory-bound passes are
    _HIPBatchNorm's kernels; each direction adds one small launch and one
    collective.  Every rank adds the same rows in rank order, so the saved
    and running statistics are bitwise rank-identical.  weight/bias
    gradients are the LOCAL sums — the DDP bucket all-reduce averages them
    like every other parameter.  The DDPX_BNFUSE producer box is not
    offered and DDPX_BN1PASS does not apply (both need the un-split
    combine)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, fuse_relu, residual, pre_stats, group, native):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        rb = None if residual is None else _chlast(_to_bf16(residual))
        row = ext.bn_sync_local(xb, pre_stats)
        gathered = _gather_rows(row, group, native)
        y, save_mean, save_invstd, mask, count = ext.bn_sync_fwd(
            xb, gathered, weight.detach(), bias.detach(), running_mean,
            running_var, momentum, eps, fuse_relu, rb)
        ctx.save_for_backward(xb, weight, save_mean, save_invstd, mask, count)
        ctx.fuse_relu = fuse_relu
        ctx.x_dtype = x.dtype
        ctx.has_residual = residual is not None
        ctx.group = group
        ctx.native = native
        # skip-grad fusion arming, exactly as _HIPBatchNorm
        ctx.skip_armed = False
        if (residual is not None and residual.is_cuda
                and residual.dtype == torch.bfloat16 and _skipfuse_on()
                and residual.requires_grad):
            sb = getattr(residual, "_ddpx_skipbox", None)
            if sb is not None:
                ctx.skip_armed = True
                ctx.skip_stash = sb
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, weight, save_mean, save_invstd, mask, count = ctx.saved_tensors
        ext = require_ext_for(dy)
        dyb = _chlast(_to_bf16(dy))
        row = ext.bn_sync_bwd_local(xb, dyb, save_mean, save_invstd, mask,
                                    ctx.fuse_relu)
        gathered = _gather_rows(row, ctx.group, ctx.native)
        out = ext.bn_sync_bwd_dx(xb, dyb, weight.detach(), save_mean,
                                 save_invstd, mask, ctx.fuse_relu, gathered,
                                 count, ctx.has_residual)
        C = weight.numel()
        dx, dbias, dweight = out[0], row[:C], row[C:]
        dresid = out[1] if ctx.has_residual else None
        if ctx.x_dtype == torch.float32:
            dx = dx.float()
        if dresid is not None and ctx.skip_armed:
            stash = ctx.skip_stash
            prev = stash.get("g")
            stash["g"] = dresid if prev is None else prev + dresid
            dresid = None   # delivered through the junction conv's dgrad
        return (dx, dweight, dbias, None, None, None, None, None, dresid,
                None, None, None)


def _count_slots(n: int, like: torch.Tensor) -> torch.Tensor:
    """The local row count as two exact fp32 values (n >> 12, n & 4095)."""
    return torch.tensor([n >> 12, n & 4095], dtype=torch.float32,
                        device=like.device)


class _TorchSyncBatchNorm(torch.autograd.Function):
    """Plain-torch SyncBatchNorm for CPU tensors (and GPU bring-up runs
    without the extension): the HIP path's formulae — local sum / sumsq /
    count rows, one gather, rank-order adds — over ``dist`` collectives."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, group):
        C = x.shape[1]
        dims = [d for d in range(x.dim()) if d != 1]
        n = x.numel() // C
        row = torch.cat([x.sum(dims), (x * x).sum(dims), _count_slots(n, x)])
        gathered = _gather_rows(row, group, None)
        tot = gathered[0].clone()
        for w in range(1, gathered.shape[0]):
            tot += gathered[w]
        M = int(tot[2 * C].item()) * 4096 + int(tot[2 * C + 1].item())
        mean = tot[:C] / M
        var = (tot[C:2 * C] / M - mean * mean).clamp_min(0)
        invstd = torch.rsqrt(var + eps)
        if running_mean is not None:
            unbiased = var * M / (M - 1) if M > 1 else var
            running_mean.mul_(1 - momentum).add_(momentum * mean)
            running_var.mul_(1 - momentum).add_(momentum * unbiased)
        shape = [1, C] + [1] * (x.dim() - 2)
        xhat = (x - mean.view(shape)) * invstd.view(shape)
        ctx.save_for_backward(xhat, weight, invstd)
        ctx.M, ctx.group, ctx.dims, ctx.shape = M, group, dims, shape
        return xhat * weight.view(shape) + bias.view(shape)

    @staticmethod
    def backward(ctx, dy):
        xhat, weight, invstd = ctx.saved_tensors
        dims, shape, M = ctx.dims, ctx.shape, ctx.M
        dbias = dy.sum(dims)
        dweight = (dy * xhat).sum(dims)
        gathered = _gather_rows(torch.cat([dbias, dweight]), ctx.group, None)
        tot = gathered[0].clone()
        for w in range(1, gathered.shape[0]):
            tot += gathered[w]
        C = weight.numel()
        a = (weight * invstd).view(shape)
        b = (tot[:C] / M).view(shape)
        c = (tot[C:] / M).view(shape)
        dx = a * (dy - b - xhat * c)
        return dx, dweight, dbias, None, None, None, None, None


def sync_batch_norm(x, running_mean, running_var, weight, bias, momentum,
                    eps, group=None, native=None, fuse_relu=False,
                    residual=None, pre_stats=None):
    """Training-mode batch_norm whose statistics span every rank of
    ``group`` (same epilogue fusions as ``batch_norm``).  Callers route
    eval mode and world size 1 to ``batch_norm`` instead."""
    if x.is_cuda and require_ext_for(x) is not None:
        return _HIPSyncBatchNorm.apply(
            x, weight, bias, running_mean, running_var, momentum, eps,
            fuse_relu, residual, pre_stats, group, native)
    xf = x.float() if x.dtype != torch.float32 else x
    y = _TorchSyncBatchNorm.apply(xf, weight, bias, running_mean,
                                  running_var, momentum, eps, group)
    if residual is not None:
        y = y + residual.float()
    if fuse_relu:
        y = F.relu(y)
    return y.to(x.dtype) if x.is_cuda and amp_mod.is_enabled() else y


class _HIPBatchNormReluPool2(torch.autograd.Function):
    """Training BatchNorm2d + fused ReLU + MaxPool2d(2) as one op.

    The forward writes only the pooled activation and one code byte per
    pooled element (window argmax + the winner's relu bit); the backward
    rebuilds the full-resolution dy_eff from the pooled dy and the code.
    Neither the full-resolution y, its relu mask nor its gradient is ever
    materialised.  Pooled y is bit-identical to batch_norm(fuse_relu) ->
    max_pool2d(2)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, pre_stats=None):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        y, save_mean, save_invstd, code = ext.bn_fwd_train_pool2(
            xb, weight.detach(), bias.detach(), running_mean, running_var,
            momentum, eps, pre_stats)
        ctx.save_for_backward(xb, weight, save_mean, save_invstd, code)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, weight, save_mean, save_invstd, code = ctx.saved_tensors
        ext = require_ext_for(dy)
        dx, dweight, dbias = ext.bn_bwd_pool2(
            xb, _chlast(_to_bf16(dy)), weight.detach(), save_mean,
            save_invstd, code)
        if ctx.x_dtype == torch.float32:
            dx = dx.float()
        return dx, dweight, dbias, None, None, None, None, None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _bn_pool_fusable(bn_mod, pool_mod, x) -> bool:
    """True when bn_mod(x) -> pool_mod may run as the fused
    BN+ReLU+pool2 kernels: training BN2d with fused ReLU feeding a plain
    2x2/stride-2 max-pool over even extents, with no opt-in that needs the
    full-resolution activation."""
    if os.environ.get("DDPX_BNPOOL", "1") == "0":
        return False
    if getattr(bn_mod, "is_sync_bn", False):
        # the junction kernels embed the un-split combine; a SyncBatchNorm
        # runs the unfused pool(bn(conv(x))) (sync-aware junction kernels
        # are a follow-up)
        return False
    if (os.environ.get("DDPX_BN1PASS", "0") == "1"
            or os.environ.get("DDPX_BNFUSE", "0") == "1"):
        return False
    if not (x.is_cuda and x.dim() == 4 and require_ext_for(x) is not None):
        return False
    if not (bn_mod.training and getattr(bn_mod, "fuse_relu", False)
            and bn_mod.track_running_stats and bn_mod.weight is not None
            and bn_mod.bias is not None):
        return False
    C, H, W = x.shape[1], x.shape[2], x.shape[3]
    if C % 8 != 0 or C // 8 > 256 or H % 2 != 0 or W % 2 != 0:
        return False
    stride = pool_mod.stride if pool_mod.stride is not None \
        else pool_mod.kernel_size
    return (isinstance(pool_mod, torch.nn.MaxPool2d)
            and _pair(pool_mod.kernel_size) == (2, 2)
            and _pair(stride) == (2, 2)
            and _pair(pool_mod.padding) == (0, 0)
            and _pair(pool_mod.dilation) == (1, 1)
            and not pool_mod.ceil_mode and not pool_mod.return_indices)


def _bn_relu_pool2(bn_mod, x, pre_stats=None):
    """The fused junction, with the module bookkeeping _bn_forward does."""
    bn_mod._check_input_dim(x)
    if bn_mod.num_batches_tracked is not None:
        bn_mod.num_batches_tracked.add_(1)
    momentum = bn_mod.momentum if bn_mod.momentum is not None else 0.1
    return _HIPBatchNormReluPool2.apply(
        x, bn_mod.weight, bn_mod.bias, bn_mod.running_mean,
        bn_mod.running_var, momentum, bn_mod.eps, pre_stats)


# ---------------------------------------------------------------- pooling ---

class _HIPMaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        y, idx = ext.maxpool2x2_fwd(xb)
        ctx.save_for_backward(idx)
        ctx.x_shape = xb.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        ext = require_ext_for(dy)
        dx = ext.maxpool2x2_bwd(_chlast(_to_bf16(dy)), idx,
                                ctx.x_shape[2], ctx.x_shape[3])
        return dx


class _HIPMaxPool(torch.autograd.Function):
    """General max pool (kernel ks, stride st, padding pad) — ResNet stem."""

    @staticmethod
    def forward(ctx, x, ks, st, pad):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        y, idx = ext.maxpool_fwd(xb, ks, st, pad)
        ctx.save_for_backward(idx)
        ctx.meta = (xb.shape[2], xb.shape[3], ks, st, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        H, W, ks, st, pad = ctx.meta
        ext = require_ext_for(dy)
        dx = ext.maxpool_bwd(_chlast(_to_bf16(dy)), idx, H, W, ks, st, pad)
        return dx, None, None, None


def max_pool2d(x, kernel_size=2, stride=None, padding=0):
    ks = kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size
    st = stride or ks
    st = st[0] if isinstance(st, (tuple, list)) else st
    pad = padding[0] if isinstance(padding, (tuple, list)) else padding
    if x.is_cuda and require_ext_for(x) is not None:
        # the dedicated 2x2 kernels need even extents; an odd last row or
        # column (dropped by floor-mode pooling) goes to the general kernel
        if (ks == 2 and st == 2 and pad == 0
                and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0):
            return _HIPMaxPool2x2.apply(x)
        return _HIPMaxPool.apply(x, ks, st, pad)
    return F.max_pool2d(x, kernel_size, stride, padding)


class _HIPGlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = require_ext_for(x)
        xb = _chlast(_to_bf16(x))
        ctx.hw = (xb.shape[2], xb.shape[3])
        return ext.global_avgpool_fwd(xb)

    @staticmethod
    def backward(ctx, dy):
        ext = require_ext_for(dy)
        return ext.global_avgpool_bwd(_to_bf16(dy.contiguous()), *ctx.hw)


def global_avg_pool2d(x):
    """[N,C,H,W] -> [N,C] mean over H,W (ResNet head: adaptive avgpool 1x1
    + flatten in one op)."""
    if x.is_cuda and require_ext_for(x) is not None:
        return _HIPGlobalAvgPool.apply(x)
    return x.float().mean(dim=(2, 3)).to(x.dtype) \
        if x.is_cuda and amp_mod.is_enabled() else x.mean(dim=(2, 3))


def relu(x, inplace=False):
    # standalone ReLU (non-fused path); fused into BN epilogue on GPU
    return F.relu(x, inplace=inplace)


class _HIPFlattenNHWC(torch.autograd.Function):
    """[N,C,H,W] channels_last bf16 -> [N, C*H*W] in NCHW semantic order
    (the reference fc1 weight layout, reference utils/model.py:23-25) with
    coalesced HIP transposes both ways — replaces ATen's strided
    permute-copies at the conv->dense junction."""

    @staticmethod
    def forward(ctx, x):
        ext = require_ext_for(x)
        ctx.chw = (x.shape[1], x.shape[2], x.shape[3])
        return ext.nhwc_flatten(x)

    @staticmethod
    def backward(ctx, dy):
        ext = require_ext_for(dy)
        return ext.nhwc_unflatten(dy.contiguous(), *ctx.chw)


def nhwc_flatten(x):
    if require_ext_for(x) is not None:
        return _HIPFlattenNHWC.apply(x)
    return torch.flatten(x, 1)


# ------------------------------------------------------------ cross entropy ---

class _HIPCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        ext = require_ext_for(logits)
        lb = logits.contiguous()
        loss, lse = ext.ce_fwd(lb, target)
        ctx.save_for_backward(lb, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        ext = require_ext_for(logits)
        dlogits = ext.ce_bwd(logits, target, lse, dloss.contiguous())
        return dlogits, None


class MixedTarget:
    """A target pair with a per-row weight: row i is class ``a[i]`` with
    weight ``lam[i]`` and class ``b[i]`` with weight ``1 - lam[i]`` (CutMix,
    or a mixup of the caller's own).  ``a``/``b`` int64 [B], ``lam`` fp32 [B]."""

    __slots__ = ("a", "b", "lam")

    def __init__(self, a, b, lam):
        self.a, self.b, self.lam = a, b, lam

    def to(self, device=None, non_blocking: bool = False):
        kw = dict(device=device, non_blocking=non_blocking)
        return MixedTarget(self.a.to(dtype=torch.long, **kw),
                           self.b.to(dtype=torch.long, **kw),
                           self.lam.to(dtype=torch.float32, **kw))

    def dominant(self) -> torch.Tensor:
        """The class that carries at least half of the weight (accuracy is
        counted against it)."""
        return torch.where(self.lam >= 0.5, self.a, self.b)

    def __len__(self):
        return self.a.shape[0]

    def __repr__(self):
        return f"MixedTarget(a={self.a}, b={self.b}, lam={self.lam})"


class _HIPMixCrossEntropy(torch.autograd.Function):
    """CE against q = eps/C + (1-eps)(lam*onehot(a) + (1-lam)*onehot(b));
    no gradient to the targets or to lam."""

    @staticmethod
    def forward(ctx, logits, a, b, lam, smoothing):
        ext = require_ext_for(logits)
        lb = logits.contiguous()
        loss, lse = ext.ce_mix_fwd(lb, a, b, lam, smoothing)
        ctx.save_for_backward(lb, a, b, lam, lse)
        ctx.smoothing = smoothing
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, a, b, lam, lse = ctx.saved_tensors
        ext = require_ext_for(logits)
        dlogits = ext.ce_mix_bwd(logits, a, b, lam, lse, dloss.contiguous(),
                                 ctx.smoothing)
        return dlogits, None, None, None, None


_ONES_CACHE: dict = {}


def _ones_f32(n: int, device) -> torch.Tensor:
    """Cached all-ones fp32 [n] (lam of a hard target); never written."""
    key = (n, device)
    t = _ONES_CACHE.get(key)
    if t is None:
        if len(_ONES_CACHE) >= 16:
            _ONES_CACHE.clear()
        t = _ONES_CACHE[key] = torch.ones(n, dtype=torch.float32,
                                          device=device)
    return t


def cross_entropy_loss(logits, target, label_smoothing: float = 0.0):
    """Mean-reduced CE (the engine applies the reference's extra /B on top —
    reference utils/process.py:22-23).

    ``target`` is an int64 class tensor or a ``MixedTarget``; with
    ``label_smoothing`` = eps the target distribution of row i is
    ``eps/C + (1-eps)*(lam_i*onehot(a_i) + (1-lam_i)*onehot(b_i))``.  A
    tensor target without smoothing takes the plain hard-target kernels."""
    eps = float(label_smoothing)
    mixed = isinstance(target, MixedTarget)
    if not mixed and eps == 0.0:
        if logits.is_cuda and require_ext_for(logits) is not None:
            return _HIPCrossEntropy.apply(logits, target)
        return F.cross_entropy(logits.float(), target)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {eps}")
    if mixed:
        a, b, lam = target.a, target.b, target.lam
    else:
        a = b = target
        lam = None
    if logits.is_cuda and require_ext_for(logits) is not None:
        if lam is None:
            lam = _ones_f32(logits.shape[0], logits.device)
        return _HIPMixCrossEntropy.apply(logits, a, b, lam, eps)
    x = logits.float()
    ce_a = F.cross_entropy(x, a, reduction="none", label_smoothing=eps)
    if lam is None:
        return ce_a.mean()
    ce_b = F.cross_entropy(x, b, reduction="none", label_smoothing=eps)
    lam = lam.to(torch.float32)
    return (lam * ce_a + (1.0 - lam) * ce_b).mean()


def argmax_correct(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Number of rows whose argmax equals target — device-side i64 scalar."""
    if logits.is_cuda and require_ext_for(logits) is not None:
        ext = require_ext_for(logits)
        return ext.argmax_correct(logits.contiguous(), target)
    return (torch.argmax(logits, dim=1) == target).sum()


def _grad_list(tensors_or_params):
    if torch.is_tensor(tensors_or_params):
        tensors_or_params = [tensors_or_params]
    out = []
    for t in tensors_or_params:
        if isinstance(t, torch.nn.Parameter):
            t = t.grad
        if t is not None:
            out.append(t)
    return out


def num_chunks(tensors, ext) -> int:
    """Partials needed by the multi-tensor square-sum kernels: one per
    (tensor, MT_CHUNK-element chunk)."""
    ch = ext.MT_CHUNK
    return sum((t.numel() + ch - 1) // ch for t in tensors)


def clip_grad_norm_impl(tensors, max_norm: float, found_inf=None, stats=None,
                        out=None, partials=None, presummed: bool = False,
                        scale: bool = True):
    """Global 2-norm clip over ``tensors`` (gradients themselves), in place.

    out[0] = norm, out[1] = clip coefficient =
    ``min(1, max_norm / (norm + 1e-6))`` (torch's clip_grad_norm_ formula) —
    1.0 when ``max_norm <= 0``, the norm is non-finite or ``found_inf`` is
    set.  ``stats`` is the 4-float telemetry buffer {sum of finite norms,
    max finite norm, #clipped steps, #finite steps}.  No host sync.
    Returns ``out`` (2 floats on the tensors' device).

    GPU: square-sum -> finalize -> in-place scale HIP kernels
    (``presummed``: ``partials`` already hold the chunk sums, from the fused
    unscale; ``scale=False`` leaves the tensors alone — the lazy clip).
    CPU: the same formula with torch ops, the sum of squares accumulated in
    float64 — the oracle for the GPU kernels."""
    max_norm = float(max_norm or 0.0)
    dev = tensors[0].device if tensors else (
        out.device if out is not None else torch.device("cpu"))
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=dev)
    ext = require_ext_for(tensors[0]) if tensors and tensors[0].is_cuda \
        else None
    if ext is not None:
        n = num_chunks(tensors, ext)
        if partials is None:
            partials = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        if not presummed:
            ext.multi_tensor_sqsum(tensors, partials)
        ext.norm_finalize(partials, n, max_norm, found_inf, out, stats)
        if scale and max_norm > 0:
            ext.multi_tensor_scale(tensors, out[1:2], found_inf)
        return out
    sq = torch.zeros((), dtype=torch.float64, device=dev)
    for t in tensors:
        sq = sq + t.detach().double().pow(2).sum()
    norm = sq.sqrt().float()
    ok = torch.isfinite(norm)
    if found_inf is not None:
        ok = ok & (found_inf.reshape(()) == 0)
    one = torch.ones((), dtype=torch.float32, device=dev)
    coef = one
    if max_norm > 0:
        coef = torch.where(ok, (max_norm / (norm + 1e-6)).clamp(max=1.0), one)
    out[0] = norm
    out[1] = coef
    if stats is not None:
        okf = ok.float()
        # where(), not multiply: a non-finite norm must leave stats untouched
        stats[0] += torch.where(ok, norm, torch.zeros_like(norm))
        stats[1] = torch.where(ok, torch.maximum(stats[1], norm), stats[1])
        stats[2] += okf * (coef < 1).float()
        stats[3] += okf
    if scale and max_norm > 0:
        with torch.no_grad():
            for t in tensors:
                t.mul_(coef)
    return out


def clip_grad_norm_(tensors_or_params, max_norm: float) -> torch.Tensor:
    """Clip the global gradient 2-norm to ``max_norm`` in place; returns the
    pre-clip norm as a 0-dim tensor on the gradients' device (no host sync).

    Accepts gradient tensors, or Parameters (their ``.grad`` is clipped).
    ``max_norm <= 0`` only measures.  Same formula as
    ``torch.nn.utils.clip_grad_norm_`` (2-norm only); on GPU it runs three
    multi-tensor HIP launches instead of ATen foreach passes."""
    return clip_grad_norm_impl(_grad_list(tensors_or_params), max_norm)[0]


def conv_bn(conv_mod, bn_mod, x, residual=None, pool=None):
    """Fused producer/consumer: on the GPU training path the conv epilogue
    emits the BN's per-channel partial statistics, and the BN forward skips
    its stats pass (SURVEY §7 M5 fusion note).  Falls back to the plain
    composition on CPU, in eval mode, or off the MFMA path.

    pool: the MaxPool2d module that consumes the BN output, if any.  A
    training BN(fuse_relu) -> MaxPool2d(2) junction over even extents runs
    as the fused BN+ReLU+pool2 kernels (``DDPX_BNPOOL=0`` opts out);
    anything else is exactly ``pool(bn(conv(x)))``."""
    use_stats = (x.is_cuda and require_ext_for(x) is not None
                 and bn_mod.training and getattr(conv_mod, "dilation",
                                                 (1, 1)) in ((1, 1), 1))
    stats = None
    if use_stats:
        stride = _uniform(conv_mod.stride, "stride")
        padding = _uniform(conv_mod.padding, "padding")
        y, stats = _HIPConv2dStats.apply(x, conv_mod.weight, conv_mod.bias,
                                         stride, padding)
    else:
        y = conv_mod(x)
    if (pool is not None and residual is None
            and _bn_pool_fusable(bn_mod, pool, y)):
        return _bn_relu_pool2(bn_mod, y, stats)
    if use_stats:
        out = bn_mod(y, residual=residual, pre_stats=stats)
    else:
        out = bn_mod(y, residual=residual)
    return out if pool is None else pool(out)
