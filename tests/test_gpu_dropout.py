"""Exact tests of the fused dropout kernels (style of test_gpu_exact.py).

Inputs are small integers that bf16 holds exactly (activations in {-2..2},
weights in {-1, 0, 1}, integer fp32 biases), so while the sum of |terms|
stays below 2^24 the fp32 accumulation is exact in any order and any split.
The expected output is built on the CPU from the numpy mirror of the mask
(``dropout_mask``) with the kernels' arithmetic reproduced in torch: one
fp32 multiply by ``scale``, one round-to-nearest-even to bf16.  Every
comparison is ``torch.equal``; nothing here has a tolerance.

Shapes (M, N, K) of the fused linear, one per route of launch_gemm_tn /
linear_act_fwd in gemm.hip:
  (1, 17, 8)      smallest GEMM route (N > 16), one partial tile
  (129, 127, 65)  just over a tile; N % 4 != 0, hash groups straddle rows
  (100, 70, 130)  split-K, S = 2: the epilogue runs in the combine kernel
  (64, 40, 1000)  S = 8 with a ragged last split
  (33, 10, 24)    N <= 16: small-N kernel + elementwise relu_dropout_fwd
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from ddp_tricks_amd import ops
from ddp_tricks_amd.ops import functional as Fo
from ddp_tricks_amd.ops.functional import (dropout_mask, dropout_scale,
                                           dropout_threshold)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

BF = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)
SEED = 0xC0FFEE1234567891        # top bit set: exercises the int64 passing
SHAPES = [(1, 17, 8), (129, 127, 65), (100, 70, 130), (64, 40, 1000),
          (33, 10, 24)]
PS = [0.0, 0.1, 0.5, 0.75]


@pytest.fixture(autouse=True)
def _fresh_rng():
    saved = ops.dropout_rng.state_dict()
    ops.dropout_rng.seed(1234, rank=0)
    yield
    ops.dropout_rng.load_state_dict(saved)


def _ints(shape, lo, hi, *key):
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, lo, hi, key))
                                                 .encode()))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _i64(seed):
    return Fo._seed_i64(seed)


def _keep(seed, shape, thr):
    n = int(np.prod(shape))
    return torch.from_numpy(dropout_mask(seed, n, thr)).view(*shape)


def _scaled_bf16(v64, scale):
    """bf16_rne(float32(v) * scale): the kernels' value arithmetic."""
    return (v64.to(torch.float32) * torch.tensor(scale, dtype=torch.float32)
            ).to(BF)


@functools.lru_cache(maxsize=None)
def _lin_case(shape):
    """Inputs and the float64 pre-activations, once per shape (read-only)."""
    M, N, K = shape
    x = _ints((M, K), -2, 2, "x")
    w = _ints((N, K), -1, 1, "w")
    b = _ints((N,), -3, 3, "b")
    acc = x @ w.t()
    absacc = x.abs() @ w.abs().t()
    assert (absacc + b.abs()).max().item() < EXACT_LIMIT
    return x, w, b, acc


def _expected_fwd(pre64, seed, thr):
    keep = _keep(seed, pre64.shape, thr)
    y = _scaled_bf16(pre64.clamp_min(0), dropout_scale(thr))
    return torch.where(keep, y, torch.zeros_like(y)), keep


# ------------------------------------------------------- fused linear fwd ---

@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_act_fwd_exact(shape, p, bias):
    x, w, b, acc = _lin_case(shape)
    thr = dropout_threshold(p)
    pre = acc + b if bias else acc
    want, keep = _expected_fwd(pre, SEED, thr)
    got = ext.linear_act_fwd(x.to(BF).to(DEV), w.to(BF).to(DEV),
                             b.float().to(DEV) if bias else None, thr,
                             dropout_scale(thr), _i64(SEED))
    assert got.dtype == BF and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    # dropped elements are +0, not -0
    assert not torch.signbit(got.cpu()[~keep]).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_p_zero_is_relu_of_linear_fwd(shape):
    x, w, b, _ = _lin_case(shape)
    xb, wb, bf = x.to(BF).to(DEV), w.to(BF).to(DEV), b.float().to(DEV)
    got = ext.linear_act_fwd(xb, wb, bf, 0, 1.0, _i64(SEED))
    assert torch.equal(got, torch.relu(ext.linear_fwd(xb, wb, bf)))


def test_bad_arguments_are_refused():
    x, w, b, _ = _lin_case((1, 17, 8))
    xb, wb = x.to(BF).to(DEV), w.to(BF).to(DEV)
    for thr, scale in ((-1, 1.0), (65536, 2.0), (0, 2.0)):
        with pytest.raises(RuntimeError):
            ext.linear_act_fwd(xb, wb, None, thr, scale, 1)
        with pytest.raises(RuntimeError):
            ext.dropout_fwd(xb, thr, scale, 1)


# ------------------------------------------------------ relu_drop_bwd ---

@pytest.mark.parametrize("scale", [2.0, dropout_scale(6554)])
@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_relu_drop_bwd_exact(n, scale):
    dy = _ints((n,), -3, 3, "dy")
    # positives, +0, -0 and negatives (a negative y never comes out of the
    # forward; it must read as "not kept" all the same)
    cycle = torch.tensor([1.0, 0.0, -0.0, -2.0, 0.5, -1.0, 3.0],
                         dtype=torch.float64)
    y = cycle.repeat(n // 7 + 1)[:n].clone()
    yb = y.to(BF)
    assert n < 7 or bool((yb < 0).any() and torch.signbit(yb[yb == 0]).any()
                         and (~torch.signbit(yb[yb == 0])).any())
    got = ext.relu_drop_bwd(dy.to(BF).to(DEV), yb.to(DEV), scale)
    want = torch.where(y > 0, _scaled_bf16(dy, scale),
                       torch.zeros(n, dtype=BF))
    assert torch.equal(got.cpu(), want)
    assert not torch.signbit(got.cpu()[~(y > 0)]).any()


# ----------------------------------------------------------- autograd ---

@pytest.mark.parametrize("p", [0.5, 0.75])
@pytest.mark.parametrize("shape", [(129, 127, 65), (100, 70, 130)])
def test_linear_act_autograd_exact(shape, p):
    """dx, dw, db of _HIPLinearAct against float64 with the same mask; the
    power-of-two scale keeps every value an integer."""
    M, N, K = shape
    x, w, b, acc = _lin_case(shape)
    dy = _ints((M, N), -2, 2, "dy")
    thr = dropout_threshold(p)
    scale = dropout_scale(thr)
    assert scale in (2.0, 4.0)
    pre = acc + b
    keep = _keep(SEED, (M, N), thr)
    dz = torch.where(keep & (pre > 0), dy * scale, torch.zeros_like(dy))
    dx_ref, dw_ref, db_ref = dz @ w, dz.t() @ x, dz.sum(0)
    assert (dz.abs() @ w.abs()).max().item() < EXACT_LIMIT
    assert (dz.abs().t() @ x.abs()).max().item() < EXACT_LIMIT
    assert dz.abs().sum(0).max().item() < EXACT_LIMIT

    xg = x.to(BF).to(DEV).requires_grad_()
    wg = w.float().to(DEV).requires_grad_()
    bg = b.float().to(DEV).requires_grad_()
    Fo.clear_weight_cache()
    y = Fo._HIPLinearAct.apply(xg, wg, bg, thr, scale, _i64(SEED))
    assert torch.equal(y.detach().cpu(), _expected_fwd(pre, SEED, thr)[0])
    y.backward(dy.to(BF).to(DEV))
    assert torch.equal(xg.grad.cpu(), dx_ref.float().to(BF))
    assert wg.grad.dtype == torch.float32
    assert torch.equal(wg.grad.cpu().double(), dw_ref)
    assert torch.equal(bg.grad.cpu().double(), db_ref)


# -------------------------------------------------- standalone dropout ---

def _standalone_inputs(dtype):
    cases = [(_ints((n,), -3, 3, "sx", n) + (0.5 if dtype is not BF else 0))
             for n in (1, 3, 8, 4099)]
    cl = _ints((2, 10, 3, 3), -3, 3, "cl") \
        .contiguous(memory_format=torch.channels_last)
    return [c.to(dtype) for c in cases] + [cl.to(dtype)]


def _storage(t):
    """The tensor's elements in storage order."""
    if t.dim() == 4 and not t.is_contiguous():
        return t.permute(0, 2, 3, 1).reshape(-1)
    return t.reshape(-1)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [BF, torch.float32],
                         ids=["bf16", "fp32"])
def test_standalone_dropout_exact(dtype, p):
    thr = dropout_threshold(p)
    scale = dropout_scale(thr)
    for x in _standalone_inputs(dtype):
        keep = torch.from_numpy(dropout_mask(SEED, x.numel(), thr))
        xd = x.to(DEV)
        y = ext.dropout_fwd(xd, thr, scale, _i64(SEED))
        assert y.dtype == dtype and y.shape == x.shape
        assert y.stride() == x.stride()
        scaled = (_storage(x).float()
                  * torch.tensor(scale, dtype=torch.float32)).to(dtype)
        want = torch.where(keep, scaled, torch.zeros_like(scaled))
        assert torch.equal(_storage(y.cpu()), want)
        # the backward regenerates the forward's mask
        ones = torch.ones_like(xd)
        f1 = ext.dropout_fwd(ones, thr, scale, _i64(SEED))
        b1 = ext.dropout_bwd(ones, thr, scale, _i64(SEED))
        assert torch.equal(f1, b1)
        assert torch.equal(_storage(f1.cpu()) != 0, keep)
        # relu variant: the N <= 16 composition's second half
        r = ext.relu_dropout_fwd(xd, thr, scale, _i64(SEED))
        rs = (_storage(x).float().clamp_min(0)
              * torch.tensor(scale, dtype=torch.float32)).to(dtype)
        assert torch.equal(_storage(r.cpu()),
                           torch.where(keep, rs, torch.zeros_like(rs)))


def test_dropout_autograd_channels_last():
    """ops.dropout through autograd: a contiguous dy is brought to the
    forward's channels_last layout before the mask is regenerated."""
    x = _ints((2, 10, 3, 3), 1, 3, "ag").to(BF).to(DEV) \
        .contiguous(memory_format=torch.channels_last).requires_grad_()
    ops.dropout_rng.set_epoch(0)
    y = ops.dropout(x, 0.5, True)
    ops.dropout_rng.set_epoch(0)
    keep = torch.from_numpy(dropout_mask(ops.dropout_rng.next_call_seed(),
                                         x.numel(), 32768))
    y.backward(torch.ones(2, 10, 3, 3, dtype=BF, device=DEV))   # NCHW dy
    assert torch.equal(_storage(y.detach().cpu()) != 0, keep)
    assert torch.equal(_storage(x.grad.cpu()), keep.to(BF) * 2)


# ------------------------------------------------------------- counter ---

def test_counter_behaviour():
    lin = ops.modules.Linear(24, 40).to(DEV)
    drop = ops.Dropout(0.5)
    x = _ints((16, 24), 1, 2, "cx").to(BF).to(DEV)

    def run():
        with torch.no_grad():
            return ops.linear_relu_dropout(lin, drop, x).cpu()

    ops.dropout_rng.seed(42, rank=0)
    ops.dropout_rng.set_epoch(3)
    a1, a2 = run(), run()
    assert not torch.equal(a1, a2)                 # two training calls differ
    ops.dropout_rng.set_epoch(3)
    b1, b2 = run(), run()
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    ops.dropout_rng.seed(42, rank=1)               # another rank salt
    ops.dropout_rng.set_epoch(3)
    assert not torch.equal(run(), a1)
    # eval: the standalone module hands its input back, nothing is drawn
    drop.eval()
    before = ops.dropout_rng.state_dict()
    assert drop(x) is x
    e1, e2 = run(), run()
    assert torch.equal(e1, e2)
    assert torch.equal(e1, torch.relu(lin(x)).detach().cpu())
    assert ops.dropout_rng.state_dict() == before


# ------------------------------------------------- default path untouched ---

def test_default_vgg_never_calls_the_dropout_kernels(monkeypatch):
    from ddp_tricks_amd.models import build_model

    def boom(*a, **k):
        raise AssertionError("dropout kernel called on the default path")

    for name in ("linear_act_fwd", "relu_drop_bwd", "dropout_fwd"):
        monkeypatch.setattr(ext, name, boom)
    from ddp_tricks_amd import amp
    amp._state.__init__()
    Fo.clear_weight_cache()
    torch.manual_seed(0)
    model = build_model("vgg16", num_classes=10, cifar_head=True,
                        dropout=0.0).to(DEV)
    model, _ = amp.initialize(model, None, opt_level="O1")
    model.train()
    before = ops.dropout_rng.state_dict()
    x = torch.rand(16, 3, 32, 32, device=DEV)
    t = torch.randint(0, 10, (16,), device=DEV)
    loss = Fo.cross_entropy_loss(model(x), t)
    loss.backward()
    torch.cuda.synchronize()
    amp._state.__init__()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None for p in model.parameters())
    assert ops.dropout_rng.state_dict() == before
