"""Exact tests of the autograd layer (ops/functional.py, ops/modules.py).

tests/test_gpu_exact.py and tests/test_gpu_norm_exact.py pin the kernels by
calling ``ext.*`` directly.  This file pins the layer ABOVE them — which
kernel runs, with which operand variant, in which layout, what is saved for
backward and which gradients are sliced, cast, stashed, summed or withheld —
and never calls ``ext.*``: every case goes through ``F_ops.conv2d``,
``F_ops.linear``, ``F_ops.max_pool2d``, ``F_ops.global_avg_pool2d``,
``F_ops.conv_bn`` / ``_HIPConv2dStats.apply`` and the ``ops.modules``
classes.

Method (sections a-d), as in test_gpu_exact.py: inputs are small integers
that bf16 holds exactly, references are float64 on the CPU, the 2^24 bound
on the reference's sum of |terms| is asserted before every comparison, and
every comparison is ``torch.equal``.  Besides values each case asserts the
output dtype, shape and memory format, and that a gradient which must not
exist is ``None`` — read off the RAW return of the backward
(``y.grad_fn.apply(dy)``), because the autograd engine silently drops a
gradient returned for an input that does not require one and silently
casts one returned in the wrong dtype.

Section d checks two small BN-free graphs end to end.  Its reference is
float64 autograd with one extra Function (``_Round``) at every op boundary
that rounds once to bf16 in forward and rounds the incoming gradient once
to bf16 in backward — exactly where the GPU path stores bf16.  Below 2^24
the fp32 value in front of each store is the exact integer, so the
roundings agree bit for bit.

Section e (residual junctions): training BN is not integer arithmetic, so
these are differential tests — one ResNet block under DDPX_SKIPFUSE=0 and 1
must give ``torch.equal`` loss, parameter gradients and input gradient,
also after a retained double backward, a no_grad forward, an abandoned
training forward, with a frozen input and with eval-mode BN.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_exact import (BF, _assert_exact_ok, _bf16_round, _ints, _nhwc,
                            _out_hw)

from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops import modules as M_ops

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32 = torch.float32

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _drop_cached_operands():
    """Every case builds its own weight tensors: do not let the operand
    cache keep them alive across the file."""
    yield
    F_ops.clear_weight_cache()


def _dev_act(t64, dtype):
    """float64 integers -> device activation: bf16 channels_last (what the
    kernels hand each other) or fp32 NCHW-contiguous (what a loader hands
    the first layer)."""
    if dtype == BF:
        return _nhwc(t64.to(BF)).to(DEV) if t64.dim() == 4 \
            else t64.to(BF).to(DEV)
    return t64.float().contiguous().to(DEV)


def _raw_backward(y, *grads):
    """The tuple the Function's backward returns, before the engine
    filters, casts or accumulates it."""
    with torch.no_grad():
        return y.grad_fn.apply(*grads)


def _is_cl(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=CL)


# masks are (x, weight, bias) requires_grad
MASKS_BIAS = [
    (True, True, True),       # everything
    (True, False, False),     # x only
    (True, False, True),      # weight frozen, bias trainable: col_sum branch
    (False, True, True),      # x needs no grad: no dgrad, no operand fetch
    (True, True, False),      # weight trainable, bias frozen
]
MASKS_NOBIAS = [(True, True, False), (True, False, False),
                (False, True, False)]


# ======================================================= a. conv routes ====

CONV_SHAPES = [
    # N, C, H, W, K, R, S, pad                    branch of _conv_fwd_prep
    (2, 1, 6, 9, 8, 3, 3, 1),     # C=1, H*W<1024: unpadded x saved, wt2_p8
    (2, 3, 9, 7, 16, 3, 3, 1),    # C=3, H*W<1024: unpadded x saved, wt2_p8
    (1, 3, 32, 32, 8, 3, 3, 1),   # C=3, H*W=1024: pad8 bwd, dw/dx[:, :C]
    (2, 8, 5, 7, 8, 3, 3, 1),     # C=8: nhwc / wt2
    (2, 16, 6, 5, 24, 3, 3, 1),   # C=16
]


def test_conv_shapes_reach_their_branches():
    use = [F_ops._use_pad8(s[1], s[2], s[3]) for s in CONV_SHAPES]
    assert use == [False, False, True, False, False]
    assert [s[1] < 8 for s in CONV_SHAPES] == [True, True, True, False, False]


@functools.lru_cache(maxsize=None)
def _conv_case(shape, stride):
    N, C, H, W, K, R, S, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    x = _ints((N, C, H, W), -2, 2, "ag x", shape)
    w = _ints((K, C, R, S), -1, 1, "ag w", shape)
    dy = _ints((N, K, P, Q), -2, 2, "ag dy", shape, stride)
    c = dict(x=x, w=w, dy=dy, P=P, Q=Q)
    c["acc"] = F.conv2d(x, w, None, stride, pad)
    c["absacc"] = F.conv2d(x.abs(), w.abs(), None, stride, pad)
    c["dx"] = torch.nn.grad.conv2d_input((N, C, H, W), w, dy, stride=stride,
                                         padding=pad)
    c["absdx"] = torch.nn.grad.conv2d_input(
        (N, C, H, W), w.abs(), dy.abs(), stride=stride, padding=pad)
    c["dw"] = torch.nn.grad.conv2d_weight(x, (K, C, R, S), dy, stride=stride,
                                          padding=pad)
    c["absdw"] = torch.nn.grad.conv2d_weight(
        x.abs(), (K, C, R, S), dy.abs(), stride=stride, padding=pad)
    c["db"] = dy.sum(dim=(0, 2, 3))
    c["absdb"] = dy.abs().sum(dim=(0, 2, 3))
    # integer biases of a few hundred push outputs past 256, onto bf16
    # rounding ties; the small ones keep sum(v^2) of the stats slab exact
    c["bias_big"] = _ints((K,), -400, 400, "ag bias", shape)
    c["bias_small"] = _ints((K,), -3, 3, "ag small bias", shape)
    return c


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", CONV_SHAPES,
                         ids=lambda s: "C%d_%dx%d" % (s[1], s[2], s[3]))
@pytest.mark.parametrize("fn", ["conv2d", "conv2d_stats"])
def test_conv_route_matrix(fn, shape, stride, monkeypatch):
    N, C, H, W, K, R, S, pad = shape
    c = _conv_case(shape, stride)
    P, Q = c["P"], c["Q"]
    bias_kinds = [None, "bias_big"] + (["bias_small"] if fn != "conv2d"
                                       else [])
    for bias_kind in bias_kinds:
        b = None if bias_kind is None else c[bias_kind]
        v = c["acc"] if b is None else c["acc"] + b.view(1, -1, 1, 1)
        absv = c["absacc"] if b is None \
            else c["absacc"] + b.abs().view(1, -1, 1, 1)
        # preconditions, on the reference alone
        _assert_exact_ok(absv)
        _assert_exact_ok(c["absdx"])
        _assert_exact_ok(c["absdw"])
        _assert_exact_ok(c["absdb"])
        sum_v, sum_v2 = v.sum(dim=(0, 2, 3)), (v * v).sum(dim=(0, 2, 3))
        _assert_exact_ok(v.abs().sum(dim=(0, 2, 3)))
        check_sq = bias_kind != "bias_big"
        if check_sq:
            _assert_exact_ok(sum_v2)
        for x_dtype in (F32, BF):
            for mask in (MASKS_NOBIAS if b is None else MASKS_BIAS):
                for wgrad_bias in (("1",) if b is None else ("1", "0")):
                    tag = (bias_kind, x_dtype, mask, wgrad_bias)
                    monkeypatch.setenv("DDPX_WGRAD_BIAS", wgrad_bias)
                    xd = _dev_act(c["x"], x_dtype).requires_grad_(mask[0])
                    wd = c["w"].float().to(DEV).requires_grad_(mask[1])
                    bd = None if b is None \
                        else b.float().to(DEV).requires_grad_(mask[2])
                    if fn == "conv2d":
                        y = F_ops.conv2d(xd, wd, bd, stride=stride,
                                         padding=pad)
                        extra = ()
                    else:
                        y, slab = F_ops._HIPConv2dStats.apply(xd, wd, bd,
                                                              stride, pad)
                        extra = (None,)
                        assert slab.dtype == F32 and not slab.requires_grad
                        assert slab.shape == (2, K, (N * P * Q + 127) // 128)
                        s = slab.double().sum(-1).cpu()
                        assert torch.equal(s[0], sum_v), tag
                        if check_sq:
                            assert torch.equal(s[1], sum_v2), tag
                    assert y.dtype == BF and y.shape == (N, K, P, Q)
                    assert _is_cl(y)
                    assert torch.equal(y.detach().cpu(), _bf16_round(v)), tag

                    dyd = _dev_act(c["dy"], BF)
                    raw = _raw_backward(y, dyd, *extra)
                    assert len(raw) == 5 and raw[3] is None and raw[4] is None
                    dx, dw, db = raw[:3]
                    if mask[0]:
                        assert dx.dtype == x_dtype, tag
                        assert dx.shape == (N, C, H, W), tag
                        if C >= 8:
                            assert _is_cl(dx)
                        want = _bf16_round(c["dx"]).to(x_dtype)
                        assert torch.equal(dx.cpu(), want), tag
                    else:
                        assert dx is None, tag
                    if mask[1]:
                        assert dw.dtype == F32 and dw.shape == (K, C, R, S)
                        assert dw.is_contiguous()
                        assert torch.equal(dw.cpu().double(), c["dw"]), tag
                    else:
                        assert dw is None, tag
                    if b is not None and mask[2]:
                        assert db.dtype == F32 and db.shape == (K,)
                        assert torch.equal(db.cpu().double(), c["db"]), tag
                    else:
                        assert db is None, tag

                    # and the engine delivers exactly those
                    y.backward(dyd)
                    for t, g in ((xd, dx), (wd, dw), (bd, db)):
                        if t is None:
                            continue
                        if g is None:
                            assert t.grad is None, tag
                        else:
                            assert t.grad.dtype == t.dtype
                            assert t.grad.shape == t.shape
                            assert torch.equal(t.grad, g), tag


# ============================================================ b. linear ====

LINEAR_SHAPES = [(5, 10, 24),     # N <= 16: the classifier-head kernels
                 (33, 17, 40)]    # general GEMM route


@pytest.mark.parametrize("mnk", LINEAR_SHAPES, ids=["head", "gemm"])
def test_linear_matrix(mnk):
    M, N, K = mnk
    x = _ints((M, K), -2, 2, "ag lin x")
    w = _ints((N, K), -1, 1, "ag lin w")
    bias = _ints((N,), -400, 400, "ag lin b")
    dy = _ints((M, N), -2, 2, "ag lin dy")
    ref_dx, ref_dw, ref_db = dy @ w, dy.t() @ x, dy.sum(0)
    _assert_exact_ok(x.abs() @ w.abs().t() + bias.abs())
    _assert_exact_ok(dy.abs() @ w.abs())
    _assert_exact_ok(dy.abs().t() @ x.abs())
    _assert_exact_ok(dy.abs().sum(0))
    for b in (None, bias):
        ref_y = x @ w.t() + (0 if b is None else b)
        for x_dtype in (F32, BF):
            for layout in ("contiguous", "transposed", "strided"):
                for mask in (MASKS_NOBIAS if b is None else MASKS_BIAS):
                    tag = (b is not None, x_dtype, layout, mask)
                    xd = _dev_act(x, x_dtype)
                    if layout == "transposed":
                        xd = xd.t().contiguous().t()
                        assert not xd.is_contiguous()
                    elif layout == "strided":
                        wide = torch.zeros(M, 2 * K, dtype=x_dtype,
                                           device=DEV)
                        wide[:, ::2] = xd
                        xd = wide[:, ::2]
                        assert not xd.is_contiguous()
                    xd = xd.detach().requires_grad_(mask[0])
                    wd = w.float().to(DEV).requires_grad_(mask[1])
                    bd = None if b is None \
                        else b.float().to(DEV).requires_grad_(mask[2])
                    y = F_ops.linear(xd, wd, bd)
                    assert y.dtype == BF and y.shape == (M, N)
                    assert y.is_contiguous()
                    assert torch.equal(y.detach().cpu(),
                                       _bf16_round(ref_y)), tag
                    dyd = _dev_act(dy, BF)
                    raw = _raw_backward(y, dyd)
                    assert len(raw) == 3
                    dx, dw, db = raw
                    if mask[0]:
                        assert dx.dtype == x_dtype and dx.shape == (M, K)
                        assert torch.equal(
                            dx.cpu(), _bf16_round(ref_dx).to(x_dtype)), tag
                    else:
                        assert dx is None, tag
                    if mask[1]:
                        assert dw.dtype == F32 and dw.shape == (N, K)
                        assert torch.equal(dw.cpu().double(), ref_dw), tag
                    else:
                        assert dw is None, tag
                    if b is not None and mask[2]:
                        assert db.dtype == F32 and db.shape == (N,)
                        assert torch.equal(db.cpu().double(), ref_db), tag
                    else:
                        assert db is None, tag
                    y.backward(dyd)
                    for t, g in ((xd, dx), (wd, dw), (bd, db)):
                        if t is None:
                            continue
                        if g is None:
                            assert t.grad is None, tag
                        else:
                            assert t.grad.dtype == t.dtype
                            assert torch.equal(t.grad, g), tag


# ================================================ c. pool / flatten / GAP ===

POOL_CASES = [
    # H, W, (kernel_size, stride, padding) as passed, 2x2 kernel expected
    (6, 8, (2, None, 0), True),            # even extents, stride=None
    (4, 4, ((2, 2), (2, 2), (0, 0)), True),    # tuple arguments
    (2, 2, (2, 2, 0), True),               # a single window
    (7, 9, (2, None, 0), False),           # odd extents: general kernel
    (7, 9, (3, 2, 1), False),              # the ResNet stem pool
    (6, 8, ((3, 3), (2, 2), (1, 1)), False),
    (6, 8, ([2, 2], None, 0), True),       # list kernel_size, stride=None
]


@pytest.mark.parametrize("case", POOL_CASES, ids=[
    "6x8_k2", "4x4_tuples", "2x2_k2s2", "7x9_k2", "7x9_k3s2p1",
    "6x8_tuples_k3s2p1", "6x8_list_k2"])
@pytest.mark.parametrize("x_dtype", ["bf16", "fp32"])
def test_max_pool2d_routing(case, x_dtype):
    H, W, (ks, st, pad), two_by_two = case
    x_dtype = BF if x_dtype == "bf16" else F32
    N, C = 2, 8
    x = _ints((N, C, H, W), -3, 3, "ag pool x")       # many ties per window
    xr = x.clone().requires_grad_(True)
    ks_ref = tuple(ks) if isinstance(ks, list) else ks
    y_ref = F.max_pool2d(xr, ks_ref, st, pad)
    dy = _ints(tuple(y_ref.shape), -2, 2, "ag pool dy", H, W, str(ks))
    y_ref.backward(dy)
    xd = _dev_act(x, x_dtype).requires_grad_(True)
    y = F_ops.max_pool2d(xd, ks, st, pad)
    want_fn = "_HIPMaxPool2x2Backward" if two_by_two else "_HIPMaxPoolBackward"
    assert type(y.grad_fn).__name__ == want_fn
    assert y.dtype == BF and y.shape == y_ref.shape and _is_cl(y)
    assert torch.equal(y.detach().cpu().double(), y_ref.detach())
    dyd = _dev_act(dy, BF)
    raw = _raw_backward(y, dyd)
    raw = raw if isinstance(raw, tuple) else (raw,)
    assert all(g is None for g in raw[1:])
    assert raw[0].dtype == BF and raw[0].shape == x.shape and _is_cl(raw[0])
    y.backward(dyd)
    assert xd.grad.dtype == x_dtype and xd.grad.shape == x.shape
    got = xd.grad.cpu().double()
    assert torch.equal(got, xr.grad)
    if (H, W) == (7, 9) and ks == 2:
        # the row and column floor-mode pooling drops get exactly zero
        assert not got[:, :, 6, :].any() and not got[:, :, :, 8].any()
        assert xr.grad[:, :, :6, :8].any()


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("C", [1, 8])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (8, 8), (10, 10)],
                         ids=lambda p: "HW%d" % (p[0] * p[1]))
def test_flatten_routing(hw, C, layout):
    H, W = hw
    N = 3
    x = _ints((N, C, H, W), -100, 100, "ag flat x")
    dy = _ints((N, C * H * W), -100, 100, "ag flat dy")
    xd = x.to(BF).to(DEV)
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=CL)
    xd.requires_grad_(True)
    y = M_ops.Flatten()(xd)
    # the kernel route: an NHWC-strided tensor at the conv->dense junction
    kernel = layout == "channels_last" and 1 < H * W <= 64 and C > 1
    assert (type(y.grad_fn).__name__ == "_HIPFlattenNHWCBackward") == kernel
    assert y.dtype == BF and y.shape == (N, C * H * W) and y.is_contiguous()
    assert torch.equal(y.detach().cpu().double(), torch.flatten(x, 1))
    y.backward(dy.to(BF).to(DEV))
    assert xd.grad.dtype == BF and xd.grad.shape == (N, C, H, W)
    assert torch.equal(xd.grad.cpu().double(), dy.view(N, C, H, W))


@pytest.mark.parametrize("x_dtype", ["bf16", "fp32"])
def test_adaptive_avg_pool_hw4(x_dtype):
    """H*W = 4: mean and gradient are multiples of 1/4, exact in bf16."""
    x_dtype = BF if x_dtype == "bf16" else F32
    N, C = 3, 8
    x = _ints((N, C, 2, 2), -3, 3, "ag gap x")
    dy = _ints((N, C, 1, 1), -3, 3, "ag gap dy")
    xd = _dev_act(x, x_dtype).requires_grad_(True)
    y = M_ops.AdaptiveAvgPool2d((1, 1))(xd)
    assert y.dtype == BF and y.shape == (N, C, 1, 1)
    assert torch.equal(y.detach().cpu().double(),
                       x.sum((2, 3), keepdim=True) / 4)
    y2 = F_ops.global_avg_pool2d(xd)
    assert y2.dtype == BF and y2.shape == (N, C) and y2.is_contiguous()
    assert torch.equal(y2.detach(), y.detach().view(N, C))
    raw = _raw_backward(y2, dy.view(N, C).to(BF).to(DEV))
    assert raw.dtype == BF and raw.shape == (N, C, 2, 2) and _is_cl(raw)
    y.backward(dy.to(BF).to(DEV))
    assert xd.grad.dtype == x_dtype and xd.grad.shape == x.shape
    assert torch.equal(xd.grad.cpu().double(), (dy / 4).expand(N, C, 2, 2))
    assert torch.equal(raw.cpu().double(), (dy / 4).expand(N, C, 2, 2))


# =========================================== d. two BN-free graphs, exact ===

class _Round(torch.autograd.Function):
    """One bf16 store: rounds once in forward and rounds the incoming
    gradient once in backward (float64 in, float64 out)."""

    @staticmethod
    def forward(ctx, t):
        return t.float().to(BF).double()

    @staticmethod
    def backward(ctx, g):
        return g.float().to(BF).double()


class _RefGraph:
    """float64 reference ops that log what the exactness bound needs."""

    def __init__(self):
        self.log = []       # (kind, input, weight, bias, raw output, args)

    def conv(self, x, w, b, stride, pad):
        y = F.conv2d(x, w, b, stride, pad)
        y.retain_grad()
        self.log.append(("conv", x.detach(), w.detach(),
                         None if b is None else b.detach(), y, (stride, pad)))
        return _Round.apply(y)

    def linear(self, x, w, b):
        y = F.linear(x, w, b)
        y.retain_grad()
        self.log.append(("linear", x.detach(), w.detach(),
                         None if b is None else b.detach(), y, ()))
        return _Round.apply(y)

    def assert_exact_ok(self):
        """Every forward output, dgrad, wgrad and bias grad of every logged
        op has sum |terms| < 2^24 (y.grad is the bf16-rounded gradient the
        GPU op receives).  Call after backward."""
        assert self.log
        for kind, x, w, b, y, args in self.log:
            g = y.grad
            assert g is not None
            xa, wa, ga = x.abs(), w.abs(), g.abs()
            if kind == "conv":
                stride, pad = args
                fwd = F.conv2d(xa, wa, None if b is None else b.abs(),
                               stride, pad)
                dgrad = torch.nn.grad.conv2d_input(
                    x.shape, wa, ga, stride=stride, padding=pad)
                wgrad = torch.nn.grad.conv2d_weight(
                    xa, w.shape, ga, stride=stride, padding=pad)
                dbias = ga.sum(dim=(0, 2, 3))
            else:
                fwd = F.linear(xa, wa, None if b is None else b.abs())
                dgrad, wgrad, dbias = ga @ wa, ga.t() @ xa, ga.sum(0)
            for t in (fwd, dgrad, wgrad, dbias):
                _assert_exact_ok(t)


def _sparse_w(shape, *key):
    """{-1, 0, 1}, mostly zero: one in four entries is drawn from
    {-1, 0, 1}, the others are 0."""
    return _ints(shape, -1, 1, "sw", *key) * \
        (_ints(shape, 0, 3, "sw keep", *key) == 0).double()


def _leaf(t64):
    return t64.clone().requires_grad_(True)


def _set(param, t64):
    with torch.no_grad():
        param.copy_(t64.float())


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """conv(C=1, bias) -> max_pool2d(2) -> conv(bias) -> Flatten -> linear
    -> linear(N=10), float64 with boundary rounding.  The hidden width 24
    takes the general GEMM route (N > 16) and keeps the head's K a
    multiple of 8, which linear_dgrad requires."""
    p = dict(
        x=_ints((2, 1, 12, 12), -2, 2, "chain x"),
        w1=_ints((8, 1, 3, 3), -1, 1, "chain w1"),     # 9 taps: dense
        b1=_ints((8,), -3, 3, "chain b1"),
        w2=_sparse_w((8, 8, 3, 3), "c2"),
        b2=_ints((8,), -300, 300, "chain b2"),
        w3=_sparse_w((24, 288), "l1"),
        b3=_ints((24,), -300, 300, "chain b3"),
        w4=_sparse_w((10, 24), "l2"),
        b4=_ints((10,), -3, 3, "chain b4"),
        dy=_ints((2, 10), -2, 2, "chain dy"),
    )
    t = {k: _leaf(v) for k, v in p.items() if k != "dy"}
    g = _RefGraph()
    h = g.conv(_Round.apply(t["x"]), t["w1"], t["b1"], 1, 1)
    h = F.max_pool2d(h, 2)
    h = g.conv(h, t["w2"], t["b2"], 1, 1)
    h = torch.flatten(h, 1)
    h = g.linear(h, t["w3"], t["b3"])
    out = g.linear(h, t["w4"], t["b4"])
    out.backward(p["dy"])
    g.assert_exact_ok()
    grads = {k: v.grad for k, v in t.items()}
    # the graph must exercise the boundary rounding, not sidestep it
    raw2 = g.log[1][4].detach()
    assert (raw2 != _bf16_round(raw2).double()).any()
    assert all(v.any() for v in grads.values())
    return p, out.detach(), grads


def test_graph_chain_exact():
    p, ref_out, ref_g = _chain_reference()
    net = torch.nn.Sequential(
        M_ops.Conv2d(1, 8, 3, padding=1), M_ops.MaxPool2d(2),
        M_ops.Conv2d(8, 8, 3, padding=1), M_ops.Flatten(),
        M_ops.Linear(288, 24), M_ops.Linear(24, 10)).to(DEV)
    for i, (w, b) in {0: ("w1", "b1"), 2: ("w2", "b2"), 4: ("w3", "b3"),
                      5: ("w4", "b4")}.items():
        _set(net[i].weight, p[w])
        _set(net[i].bias, p[b])
    x = _dev_act(p["x"], F32).requires_grad_(True)
    h = x
    routes = []
    for layer in net:
        h = layer(h)
        routes.append(type(h.grad_fn).__name__)
    assert routes == ["_HIPConv2dBackward", "_HIPMaxPool2x2Backward",
                      "_HIPConv2dBackward", "_HIPFlattenNHWCBackward",
                      "_HIPLinearBackward", "_HIPLinearBackward"]
    assert h.dtype == BF and h.shape == (2, 10)
    assert torch.equal(h.detach().cpu().double(), ref_out)
    h.backward(p["dy"].to(BF).to(DEV))
    assert x.grad.dtype == F32 and x.grad.shape == x.shape
    assert torch.equal(x.grad.cpu().double(), ref_g["x"])
    for i, (w, b) in {0: ("w1", "b1"), 2: ("w2", "b2"), 4: ("w3", "b3"),
                      5: ("w4", "b4")}.items():
        for param, key in ((net[i].weight, w), (net[i].bias, b)):
            assert param.grad.dtype == F32
            assert param.grad.shape == param.shape
            assert torch.equal(param.grad.cpu().double(), ref_g[key]), key


@functools.lru_cache(maxsize=None)
def _fanout_reference():
    """out = conv_a(x) + conv_b(x), pooled = max_pool2d(x, 2): one bf16 x
    with three consumers, two of them stride-1 convs (both attach the
    junction box)."""
    p = dict(
        x=_ints((2, 8, 6, 6), -2, 2, "fan x"),
        wa=_sparse_w((8, 8, 3, 3), "fa"),
        ba=_ints((8,), -300, 300, "fan ba"),
        wb=_ints((8, 8, 1, 1), -1, 1, "fan wb"),       # 8 taps: dense
        g_out=_ints((2, 8, 6, 6), -2, 2, "fan g out"),
        g_pool=_ints((2, 8, 3, 3), -2, 2, "fan g pool"),
    )
    t = {k: _leaf(p[k]) for k in ("x", "wa", "ba", "wb")}
    g = _RefGraph()
    # every consumer stores its own bf16 dx: one _Round per branch
    ya = g.conv(_Round.apply(t["x"]), t["wa"], t["ba"], 1, 1)
    yb = g.conv(_Round.apply(t["x"]), t["wb"], None, 1, 0)
    out = _Round.apply(ya + yb)                   # the bf16 add's store
    pooled = F.max_pool2d(_Round.apply(t["x"]), 2)
    torch.autograd.backward([out, pooled], [p["g_out"], p["g_pool"]])
    g.assert_exact_ok()
    # x.grad is the sum of the three bf16 branch gradients, accumulated in
    # bf16 in whatever order the engine picks: exact while the sum of
    # their magnitudes stays within the integers bf16 holds (<= 256)
    parts = [_bf16_round(torch.nn.grad.conv2d_input(
        x.shape, w, y.grad, stride=1, padding=args[1])).double()
        for _, x, w, _, y, args in g.log]
    xp = _leaf(p["x"])
    F.max_pool2d(xp, 2).backward(p["g_pool"])
    parts.append(xp.grad)
    assert sum(q.abs() for q in parts).max().item() <= 256
    assert all(q.any() for q in parts)
    assert torch.equal(t["x"].grad, sum(parts))
    grads = {k: v.grad for k, v in t.items()}
    return p, out.detach(), pooled.detach(), grads


def test_graph_fanout_exact():
    p, ref_out, ref_pool, ref_g = _fanout_reference()
    conv_a = M_ops.Conv2d(8, 8, 3, padding=1).to(DEV)
    conv_b = M_ops.Conv2d(8, 8, 1, bias=False).to(DEV)
    _set(conv_a.weight, p["wa"])
    _set(conv_a.bias, p["ba"])
    _set(conv_b.weight, p["wb"])
    x = _dev_act(p["x"], BF).requires_grad_(True)
    ya, yb = conv_a(x), conv_b(x)
    assert ya.grad_fn.skip_box is yb.grad_fn.skip_box     # one box on x
    out = ya + yb
    pooled = F_ops.max_pool2d(x, 2)
    assert out.dtype == BF and out.shape == (2, 8, 6, 6) and _is_cl(out)
    assert torch.equal(out.detach().cpu().double(), ref_out)
    assert torch.equal(pooled.detach().cpu().double(), ref_pool)
    torch.autograd.backward(
        [out, pooled], [_dev_act(p["g_out"], BF), _dev_act(p["g_pool"], BF)])
    assert "g" not in ya.grad_fn.skip_box                 # nothing left over
    assert x.grad.dtype == BF and x.grad.shape == x.shape
    assert torch.equal(x.grad.cpu().double(), ref_g["x"])
    for param, key in ((conv_a.weight, "wa"), (conv_a.bias, "ba"),
                       (conv_b.weight, "wb")):
        assert param.grad.dtype == F32 and param.grad.shape == param.shape
        assert torch.equal(param.grad.cpu().double(), ref_g[key]), key
    assert conv_b.bias is None


# ================================================= e. residual junctions ===

BLOCKS = ["basic", "bottleneck", "bottleneck_ds1", "bottleneck_ds2"]
SEQUENCES = ["plain", "backward_twice", "no_grad_forward_first",
             "abandoned_forward_first", "input_frozen", "bn_eval"]
BLOCK_N, BLOCK_C, BLOCK_HW = 4, 32, 6


def _make_block(kind):
    from ddp_tricks_amd.models.resnet import (BasicBlock, Bottleneck,
                                              conv1x1)
    torch.manual_seed(1234)
    if kind == "basic":
        block = BasicBlock(BLOCK_C, BLOCK_C)
    elif kind == "bottleneck":
        block = Bottleneck(BLOCK_C, 8)
    else:
        stride = 1 if kind == "bottleneck_ds1" else 2
        ds = torch.nn.Sequential(conv1x1(BLOCK_C, 32, stride),
                                 M_ops.BatchNorm2d(32))
        block = Bottleneck(BLOCK_C, 8, stride, ds)
    # non-trivial affine BN parameters and running statistics
    for m in block.modules():
        if isinstance(m, M_ops.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return block.to(DEV)


@functools.lru_cache(maxsize=None)
def _block_io(kind):
    g = torch.Generator().manual_seed(99)
    x = torch.randn(BLOCK_N, BLOCK_C, BLOCK_HW, BLOCK_HW, generator=g)
    ohw = BLOCK_HW if kind != "bottleneck_ds2" else BLOCK_HW // 2
    coef = torch.randn(BLOCK_N, 32, ohw, ohw, generator=g)
    return x, coef


def _run_block(kind, sequence, skipfuse, monkeypatch):
    """One step of the block; returns loss, block-input gradient and the
    parameter gradients (all detached clones) plus the output tensor."""
    monkeypatch.setenv("DDPX_SKIPFUSE", skipfuse)
    block = _make_block(kind)
    block.train(sequence != "bn_eval")
    x64, coef = _block_io(kind)
    x = x64.to(BF).to(DEV).contiguous(memory_format=CL)
    x.requires_grad_(sequence != "input_frozen")
    coef = coef.to(DEV)
    if sequence == "no_grad_forward_first":
        with torch.no_grad():
            block(x)
    elif sequence == "abandoned_forward_first":
        lost = (block(x).float() * coef).sum()        # never backpropagated
        assert lost.requires_grad
        del lost
    out = block(x)
    assert out.dtype == BF and _is_cl(out) and out.shape == coef.shape
    loss = (out.float() * coef).sum()
    if sequence == "backward_twice":
        loss.backward(retain_graph=True)
    loss.backward()
    names = [n for n, _ in block.named_parameters()]
    assert all(p.grad is not None and p.grad.dtype == F32
               and p.grad.shape == p.shape for p in block.parameters())
    if sequence == "input_frozen":
        assert x.grad is None
        xg = None
    else:
        assert x.grad.dtype == BF and x.grad.shape == x.shape
        xg = x.grad.detach().clone()
    box = getattr(x, "_ddpx_skipbox", None)
    assert box is None or "g" not in box                  # nothing left over
    return dict(loss=loss.detach().clone(), xg=xg, names=names,
                grads=[p.grad.detach().clone() for p in block.parameters()])


def _assert_same_step(a, b, scale=1):
    assert torch.equal(a["loss"], b["loss"])
    assert a["names"] == b["names"]
    for n, ga, gb in zip(a["names"], a["grads"], b["grads"]):
        assert torch.isfinite(ga).all() and ga.any(), n
        assert torch.equal(ga, gb * scale), n
    assert (a["xg"] is None) == (b["xg"] is None)
    if a["xg"] is not None:
        assert a["xg"].float().any()
        assert torch.equal(a["xg"], b["xg"] * scale)


@pytest.mark.parametrize("sequence", SEQUENCES)
@pytest.mark.parametrize("kind", BLOCKS)
def test_residual_junction_skipfuse_bit_equal(kind, sequence, monkeypatch):
    fused = _run_block(kind, sequence, "1", monkeypatch)
    plain = _run_block(kind, sequence, "0", monkeypatch)
    _assert_same_step(fused, plain)
    if sequence in ("no_grad_forward_first", "abandoned_forward_first"):
        # training-mode outputs and gradients do not depend on the running
        # statistics: the step equals a step with nothing before it
        for mode, got in (("1", fused), ("0", plain)):
            _assert_same_step(got, _run_block(kind, "plain", mode,
                                              monkeypatch))
    if sequence == "backward_twice":
        # accumulating the same gradient twice is an exact doubling
        for mode, got in (("1", fused), ("0", plain)):
            _assert_same_step(got, _run_block(kind, "plain", mode,
                                              monkeypatch), scale=2)


def test_residual_junction_arms_where_expected(monkeypatch):
    """The differential test above really compares two different paths:
    with fusion on, the identity blocks stash dresid in the box on x."""
    monkeypatch.setenv("DDPX_SKIPFUSE", "1")
    for kind, armed in (("basic", True), ("bottleneck", True),
                        ("bottleneck_ds1", False), ("bottleneck_ds2", False)):
        block = _make_block(kind).train()
        x = _block_io(kind)[0].to(BF).to(DEV).contiguous(memory_format=CL)
        x.requires_grad_(True)
        out = block(x)
        assert hasattr(x, "_ddpx_skipbox")        # stride-1 conv1 on x
        assert out.grad_fn.skip_armed == armed, kind
