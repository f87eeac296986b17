"""Exact-arithmetic kernel tests at tile, split and shape edges.

Every input is a small integer that bf16 represents exactly (activations
and gradients in {-2..2}, weights in {-1, 0, 1}, integer-valued fp32
biases), so every product and every partial sum is an integer.  While the
sum of |terms| stays below 2^24, fp32 accumulation is exact in ANY order:
any split-K grouping, MFMA or fmaf path and any slab combine must then
produce the mathematically exact result.  fp32 outputs are compared with
a float64 CPU reference by ``torch.equal``; bf16 outputs with that
reference rounded once to bf16 (integers above 256 land on rounding ties,
which pins round-to-nearest-even).  No comparison here has a tolerance.

Each test asserts the 2^24 precondition on the REFERENCE alone (never on
the kernel output) before it looks at the kernel.

Shapes are (N, C, H, W, K, R, S, stride, pad); each is the smallest that
reaches the edge named next to it (dispatch rules: conv2d_fwd /
conv2d_dgrad / conv2d_wgrad in conv.hip, launch_gemm_tn / linear_* /
col_sum in gemm.hip).  All tests @pytest.mark.gpu — they need an MI355X.
"""
import functools
import itertools
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

BF = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)


# ---------------------------------------------------------------- helpers ---

def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(shape, lo, hi, *key):
    """float64 CPU tensor of integers in [lo, hi], repeatable per key."""
    g = torch.Generator().manual_seed(_seed(shape, lo, hi, *key))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _nonzero_ints(shape, mag, *key):
    """Integers in [-mag, mag] with no zero."""
    v = _ints(shape, 1, mag, *key, "mag")
    s = _ints(shape, 0, 1, *key, "sign") * 2 - 1
    return v * s


def _assert_exact_ok(abs_sum):
    """The precondition: the sum of |terms| of every output element (given
    as a float64 tensor computed from the reference inputs) is < 2^24."""
    assert abs_sum.abs().max().item() < EXACT_LIMIT


def _bf16_round(ref64):
    return ref64.to(torch.float32).to(BF)


def _nhwc(t):
    """[N,C,H,W]-logical tensor whose memory is NHWC whatever the sizes."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _act(t64):
    """float64 [N,C,H,W] integers -> bf16 channels_last device tensor."""
    return _nhwc(t64.to(BF)).to(DEV)


def _out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _wt2(w64):
    """[K,C,R,S] -> the dgrad operand WT2[C, R*S*K] (bf16, device)."""
    K, C, R, S = w64.shape
    return w64.to(BF).permute(1, 2, 3, 0).reshape(C, R * S * K) \
        .contiguous().to(DEV)


# ----------------------------------------------------------- conv forward ---

FWD_SHAPES = [
    (2, 8, 5, 7, 8, 3, 3, 1, 1),      # M=70 < tile; Ko=8; Kgemm=72=64+8; H!=W
    (2, 8, 8, 8, 64, 1, 1, 1, 0),     # M = 128 exactly
    (1, 8, 3, 43, 64, 1, 1, 1, 0),    # M = 129
    (1, 16, 9, 6, 136, 3, 3, 1, 0),   # Ko = 128 + 8 tail tile
    (3, 24, 11, 13, 72, 1, 3, 1, 1),  # R != S
    (2, 8, 12, 10, 64, 3, 1, 2, 0),   # R != S with stride 2
    (3, 40, 7, 9, 192, 5, 5, 1, 2),   # Kgemm=1000; Ko=128+64; M=189
    (2, 16, 10, 13, 32, 3, 3, 3, 1),  # stride 3
    (2, 1, 6, 9, 8, 3, 3, 1, 0),      # direct C<8 kernel k_conv_small_cin
    (2, 3, 9, 7, 16, 5, 3, 2, 2),     # direct C<8 kernel
]
STATS_SHAPES = [s for s in FWD_SHAPES if s[1] % 8 == 0]


@functools.lru_cache(maxsize=None)
def _fwd_case(shape):
    """Inputs and the float64 bias-free reference, computed once per shape
    and shared (read-only) by the fwd and stats tests."""
    N, C, H, W, K, R, S, stride, pad = shape
    x = _ints((N, C, H, W), -2, 2, "x")
    w = _ints((K, C, R, S), -1, 1, "w")
    acc = F.conv2d(x, w, None, stride, pad)
    absacc = F.conv2d(x.abs(), w.abs(), None, stride, pad)
    P, Q = _out_hw(H, W, R, S, stride, pad)
    assert acc.shape == (N, K, P, Q)
    return x, w, acc, absacc


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_conv_fwd_exact(shape, with_bias):
    N, C, H, W, K, R, S, stride, pad = shape
    x, w, acc, absacc = _fwd_case(shape)
    # biases of a few hundred push outputs past 256, where bf16 spacing is
    # 2 or 4 and odd integers are rounding ties
    b = _ints((K,), -400, 400, "bias", shape) if with_bias else None
    ref = acc if b is None else acc + b.view(1, -1, 1, 1)
    _assert_exact_ok(absacc if b is None
                     else absacc + b.abs().view(1, -1, 1, 1))
    y = ext.conv2d_fwd(_act(x), _act(w),
                       None if b is None else b.float().to(DEV), stride, pad)
    assert y.shape == ref.shape and y.dtype == BF
    assert torch.equal(y.cpu(), _bf16_round(ref))


@pytest.mark.parametrize("shape", STATS_SHAPES)
def test_conv_fwd_stats_exact(shape):
    """y is bit-equal to conv2d_fwd and the slab sums equal the float64
    sum / sum of squares of the UNROUNDED acc + bias over the valid rows —
    rows past M (partial last tile) and columns past Ko add nothing."""
    N, C, H, W, K, R, S, stride, pad = shape
    x, w, acc, absacc = _fwd_case(shape)
    b = _nonzero_ints((K,), 3, "stats bias", shape)
    v = acc + b.view(1, -1, 1, 1)
    _assert_exact_ok(absacc + b.abs().view(1, -1, 1, 1))
    ref_sum = v.sum(dim=(0, 2, 3))
    ref_sq = (v * v).sum(dim=(0, 2, 3))
    _assert_exact_ok(ref_sq)            # bounds sum|v| too (integers)
    xd, wd, bd = _act(x), _act(w), b.float().to(DEV)
    y, slab = ext.conv2d_fwd_stats(xd, wd, bd, stride, pad)
    y_plain = ext.conv2d_fwd(xd, wd, bd, stride, pad)
    M = N * acc.shape[2] * acc.shape[3]
    assert slab.dtype == torch.float32
    assert slab.shape == (2, K, (M + 127) // 128)
    assert torch.equal(y, y_plain)
    assert torch.equal(y.cpu(), _bf16_round(v))
    s = slab.double().sum(-1).cpu()
    assert torch.equal(s[0], ref_sum)
    assert torch.equal(s[1], ref_sq)


def test_conv_fwd_rejects_ko_not_multiple_of_8():
    """The MFMA epilogue stores 8-channel chunks: Ko = 12 must raise."""
    x = _act(_ints((1, 8, 4, 4), -2, 2, "x12"))
    w = _act(_ints((12, 8, 3, 3), -1, 1, "w12"))
    with pytest.raises(RuntimeError):
        ext.conv2d_fwd(x, w, None, 1, 1)
    with pytest.raises(RuntimeError):
        ext.conv2d_fwd_stats(x, w, None, 1, 1)


# ------------------------------------------------------------- conv dgrad ---

DGRAD_SHAPES = [
    # the stride-1 forward cases, C and K swapped where that puts the tile
    # edge on C (the dgrad GEMM's N dimension); here M = N*H*W
    (2, 8, 5, 7, 8, 3, 3, 1, 1),      # M=70; C=8 (56 masked columns)
    (2, 64, 8, 8, 8, 1, 1, 1, 0),     # M = 128 exactly
    (1, 64, 3, 43, 8, 1, 1, 1, 0),    # M = 129
    (3, 72, 11, 13, 24, 1, 3, 1, 1),  # R != S; C = 64 + 8
    (3, 192, 7, 9, 40, 5, 5, 1, 2),   # Kgemm = 1000; C = 128 + 64
    (1, 136, 6, 5, 16, 3, 3, 1, 1),   # 128-wide tile plus tail
    (2, 16, 8, 9, 8, 3, 3, 2, 0),     # (H+2p-R) % stride != 0: last row bare
    (2, 16, 8, 10, 8, 3, 3, 2, 0),    # ... last row AND last column bare
    (2, 8, 9, 12, 16, 1, 1, 2, 0),    # s2 R=1: three empty classes, pre-zero
    (2, 8, 8, 10, 16, 2, 2, 2, 0),    # s2 R=2: one tap per class
    (2, 8, 9, 11, 8, 5, 5, 2, 2),     # s2 R=5: odd H, W -> class grids differ
    (2, 16, 10, 13, 32, 3, 3, 3, 1),  # s3 R=3: 9 classes, 4 packed + 5 single
    (2, 8, 7, 8, 8, 1, 1, 3, 0),      # s3 R=1
]


@functools.lru_cache(maxsize=None)
def _dgrad_case(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    dy = _ints((N, K, P, Q), -2, 2, "dy")
    w = _ints((K, C, R, S), -1, 1, "w")
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w, dy, stride=stride,
                                     padding=pad)
    absref = torch.nn.grad.conv2d_input((N, C, H, W), w.abs(), dy.abs(),
                                        stride=stride, padding=pad)
    return dy, w, ref, absref


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_conv_dgrad_exact(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    dy, w, ref, absref = _dgrad_case(shape)
    _assert_exact_ok(absref)
    dx = ext.conv2d_dgrad(_act(dy), _wt2(w), N, C, H, W, R, S, stride, pad)
    assert dx.shape == ref.shape and dx.dtype == BF
    dxc = dx.cpu()
    # input rows / columns that no output tap reaches must come out as
    # exact zeros (dx is allocated uninitialised)
    if (H + 2 * pad - R) % stride != 0:
        assert not ref[:, :, -1, :].any()
        assert not dxc[:, :, -1, :].any()
    if (W + 2 * pad - S) % stride != 0:
        assert not ref[:, :, :, -1].any()
        assert not dxc[:, :, :, -1].any()
    assert torch.equal(dxc, _bf16_round(ref))


def test_conv_dgrad_bare_edges_are_covered():
    """The table above really holds a bare last row and a bare last
    column (the zero checks in test_conv_dgrad_exact are conditional)."""
    rows = [s for s in DGRAD_SHAPES if (s[2] + 2 * s[8] - s[5]) % s[7] != 0]
    cols = [s for s in DGRAD_SHAPES if (s[3] + 2 * s[8] - s[6]) % s[7] != 0]
    assert rows and cols


def test_conv_dgrad_addend_exact():
    """Fused skip-grad epilogue: dx = bf16(float(bf16(ref)) + g) — rounded
    twice, exactly like the unfused dgrad followed by a bf16 add."""
    shape = (1, 136, 6, 5, 16, 3, 3, 1, 1)
    N, C, H, W, K, R, S, stride, pad = shape
    dy, w, ref, absref = _dgrad_case(shape)
    _assert_exact_ok(absref)
    # even integers up to 256 are exact in bf16 and push sums onto ties
    g = _ints((N, C, H, W), -128, 128, "addend") * 2
    assert torch.equal(g.to(BF).double(), g)
    want = (_bf16_round(ref).float() + g.float()).to(BF)
    dx = ext.conv2d_dgrad(_act(dy), _wt2(w), N, C, H, W, R, S, stride, pad,
                          _act(g))
    assert torch.equal(dx.cpu(), want)


def test_conv_dgrad_rejects_c_not_multiple_of_8():
    """The dgrad epilogue stores 8-channel chunks: C = 12 must raise."""
    dy = _act(_ints((1, 8, 4, 4), -2, 2, "dy12"))
    wt2 = _wt2(_ints((8, 12, 3, 3), -1, 1, "w12"))
    with pytest.raises(RuntimeError):
        ext.conv2d_dgrad(dy, wt2, 1, 12, 4, 4, 3, 3, 1, 1)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", [
    (2, 8, 5, 7, 8, 3, 3, 1, 1),
    (1, 136, 6, 5, 16, 3, 3, 1, 1),   # second N tile: channel groups 16..
])
def test_conv_dgrad_bn_exact(shape, masked):
    """dx bit-equal to conv2d_dgrad; slab sums equal sum(g) and
    sum(g * xhat) with g the relu-masked, bf16-ROUNDED dx.  mean is
    integer-valued and invstd a power of two, so xhat is exact."""
    N, C, H, W, K, R, S, stride, pad = shape
    dy, w, ref, absref = _dgrad_case(shape)
    _assert_exact_ok(absref)
    M = N * H * W
    bn_x = _ints((N, C, H, W), -2, 2, "bn_x")
    mean = _ints((C,), -2, 2, "bn_mean")
    invstd = 0.5 ** _ints((C,), 1, 2, "bn_invstd")      # 0.5 or 0.25
    if masked:
        mask = _ints((M, C // 8), 0, 255, "mask").to(torch.uint8)
        bits = (mask.view(N, H, W, C // 8, 1).int()
                >> torch.arange(8).int()) & 1            # bit j = ch 8*c8+j
        keep = bits.reshape(N, H, W, C).permute(0, 3, 1, 2).double()
    else:
        mask = torch.empty(0, dtype=torch.uint8)         # empty = no ReLU
        keep = torch.ones(N, C, H, W, dtype=torch.float64)
    g = _bf16_round(ref).double() * keep
    xhat = (bn_x - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    ref_sum = g.sum(dim=(0, 2, 3))
    ref_sx = (g * xhat).sum(dim=(0, 2, 3))
    # terms of sum(g*xhat) are multiples of 1/4: scale to integers first
    _assert_exact_ok(g.abs().sum(dim=(0, 2, 3)))
    _assert_exact_ok((g * xhat).abs().sum(dim=(0, 2, 3)) * 4)

    dyd, wt2 = _act(dy), _wt2(w)
    dx, slab = ext.conv2d_dgrad_bn(
        dyd, wt2, N, C, H, W, R, S, pad, _act(bn_x), mask.to(DEV),
        mean.float().to(DEV), invstd.float().to(DEV))
    dx_plain = ext.conv2d_dgrad(dyd, wt2, N, C, H, W, R, S, 1, pad)
    assert slab.dtype == torch.float32
    assert slab.shape == (2, C, (M + 127) // 128)
    assert torch.equal(dx, dx_plain)
    assert torch.equal(dx.cpu(), _bf16_round(ref))
    s = slab.double().sum(-1).cpu()
    assert torch.equal(s[0], ref_sum)
    assert torch.equal(s[1], ref_sx)


@pytest.mark.parametrize("shape", [
    (2, 1, 6, 9, 8, 3, 3, 1, 1),      # C=1, small spatial: unpadded x saved
    (2, 3, 9, 7, 16, 3, 3, 2, 1),     # C=3, stride 2
])
def test_small_cin_autograd_grads_exact(shape):
    """functional.conv2d with C < 8 and a small image saves the UNPADDED
    input for the specialised wgrad kernels; its input gradient must
    still come from the 8-channel dgrad kernel on the padded operand (the
    kernel writes 8-channel chunks) with the pad channels sliced off."""
    from ddp_tricks_amd.ops import functional as F_ops
    N, C, H, W, K, R, S, stride, pad = shape
    assert not F_ops._use_pad8(C, H, W)
    dy, w, ref, absref = _dgrad_case(shape)
    x = _ints((N, C, H, W), -2, 2, "x")
    ref_dw = torch.nn.grad.conv2d_weight(x, (K, C, R, S), dy, stride=stride,
                                         padding=pad)
    _assert_exact_ok(absref)
    _assert_exact_ok(torch.nn.grad.conv2d_weight(
        x.abs(), (K, C, R, S), dy.abs(), stride=stride, padding=pad))
    xd = x.float().to(DEV).requires_grad_(True)
    wd = torch.nn.Parameter(w.float().to(DEV))
    y = F_ops.conv2d(xd, wd, None, stride=stride, padding=pad)
    assert torch.equal(y.detach().cpu(),
                       _bf16_round(F.conv2d(x, w, None, stride, pad)))
    y.backward(_act(dy).to(y.dtype))
    assert xd.grad.shape == (N, C, H, W)
    assert torch.equal(xd.grad.cpu().double(), _bf16_round(ref).double())
    assert torch.equal(wd.grad.cpu().double(), ref_dw)


# ------------------------------------------------------------- conv wgrad ---

# shape, the leaf name conv2d_wgrad_plan must report for it, and the split
# where the row is there for it (None: not asserted)
_WGRAD_ROWS = [
    ((2, 8, 5, 7, 8, 3, 3, 1, 1), "sb_pair<64>", 1),
    ((4, 8, 64, 65, 8, 1, 1, 1, 0), "sb_pair<64>", 64),  # M=16640: S_ > 16
                                # -> two-stage combine; M % (64*64) != 0
    ((2, 8, 6, 6, 72, 3, 3, 1, 1), "sb_pair<32>", None),    # gk = 2
    ((2, 56, 6, 5, 136, 3, 3, 1, 1), "wide_dma<32>", None),  # Ko, Kgemm=504
                                                             # tails
    ((2, 128, 5, 6, 128, 3, 3, 1, 1), "wide_dma<64>", None),  # Kgemm = 1152
    ((2, 136, 5, 6, 136, 3, 3, 1, 1), "wide_dma<64>", None),  # with tails
    ((2, 16, 10, 13, 32, 3, 3, 3, 1), "sb_pair<64>", None),   # stride 3
    ((2, 8, 12, 10, 64, 3, 1, 2, 0), "sb_pair<64>", None),    # R != S
    ((1, 1, 3, 3, 8, 3, 3, 1, 0), "c1_r3_stream", 1),         # M = 1
    ((3, 1, 7, 9, 8, 3, 3, 1, 1), "c1_r3_stream", None),      # padded
    ((3, 1, 9, 8, 16, 3, 3, 2, 0), "c1_r3_stream", None),     # stride 2
    ((2, 3, 6, 8, 16, 2, 2, 1, 0), "small_rsc", None),        # rsc = 12
    ((2, 1, 7, 6, 8, 4, 4, 1, 1), "small_rsc", None),         # rsc = 16
    ((2, 3, 7, 6, 16, 3, 3, 1, 1), "small_cin", None),        # rsc = 27
    ((2, 1, 6, 7, 72, 3, 3, 1, 1), "small_cin", None),        # Ko > 64
    ((2, 3, 7, 6, 136, 3, 3, 1, 0), "small_cin", None),       # Ko > 64
]


@pytest.mark.parametrize("shape,leaf,split", _WGRAD_ROWS,
                         ids=[f"shape{i}" for i in range(len(_WGRAD_ROWS))])
def test_conv_wgrad_exact(shape, leaf, split):
    N, C, H, W, K, R, S, stride, pad = shape
    got_leaf, got_split, _ = ext.conv2d_wgrad_plan(*shape, False)
    assert got_leaf == leaf
    assert split is None or got_split == split   # 64 > 16: two-stage combine
    P, Q = _out_hw(H, W, R, S, stride, pad)
    x = _ints((N, C, H, W), -2, 2, "x")
    dy = _ints((N, K, P, Q), -2, 2, "dy")
    ref = torch.nn.grad.conv2d_weight(x, (K, C, R, S), dy, stride=stride,
                                      padding=pad)
    _assert_exact_ok(torch.nn.grad.conv2d_weight(
        x.abs(), (K, C, R, S), dy.abs(), stride=stride, padding=pad))
    dw = ext.conv2d_wgrad(_act(dy), _act(x), R, S, stride, pad)
    assert dw.dtype == torch.float32 and dw.shape == (K, C, R, S)
    assert torch.equal(dw.cpu().double(), ref)


# ------------------------------------------------------------------- GEMM ---

GEMM_SHAPES = [
    (1, 1, 1),           # smallest
    (5, 3, 7),           # smaller than one tile
    (128, 128, 64),      # exact tile
    (129, 127, 65),      # just over a tile
    (100, 70, 130),      # split-K S=2, second split holds 2 elements
    (64, 40, 1000),      # S=8 with a 104-element last split
    (16, 24, 8192),      # S=16
]


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K):
    A = _ints((M, K), -2, 2, "A")
    B = _ints((N, K), -1, 1, "B")
    bias = _ints((N,), -400, 400, "gemm bias")
    ref = A @ B.t()
    absref = A.abs() @ B.abs().t()
    return A, B, bias, ref, absref


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("mnk", GEMM_SHAPES)
def test_gemm_tn_exact(mnk, out_f32, with_bias):
    A, B, bias, ref, absref = _gemm_case(*mnk)
    if with_bias:
        ref = ref + bias
        absref = absref + bias.abs()
    _assert_exact_ok(absref)
    C = ext.gemm_tn(A.to(BF).to(DEV), B.to(BF).to(DEV),
                    bias.float().to(DEV) if with_bias else None, out_f32)
    assert C.shape == ref.shape
    if out_f32:
        assert C.dtype == torch.float32
        assert torch.equal(C.cpu().double(), ref)
    else:
        assert C.dtype == BF
        assert torch.equal(C.cpu(), _bf16_round(ref))


# ----------------------------------------------------------------- linear ---

@pytest.mark.parametrize("N", [1, 10, 16, 17])     # 17: the GEMM route
def test_linear_fwd_exact(N):
    for K, M, with_bias in itertools.product([7, 8, 9, 520], [1, 257],
                                             [False, True]):
        x = _ints((M, K), -2, 2, "lin x")
        w = _ints((N, K), -1, 1, "lin w")
        b = _ints((N,), -400, 400, "lin b")
        ref = x @ w.t() + (b if with_bias else 0)
        _assert_exact_ok(x.abs() @ w.abs().t() + b.abs())
        y = ext.linear_fwd(x.to(BF).to(DEV), w.to(BF).to(DEV),
                           b.float().to(DEV) if with_bias else None)
        assert y.dtype == BF and y.shape == (M, N)
        assert torch.equal(y.cpu(), _bf16_round(ref)), (M, N, K, with_bias)


@pytest.mark.parametrize("mnk", [
    (1, 10, 8), (300, 10, 520), (5, 16, 24), (7, 1, 8),   # k_gemm_nn_smallk
    (5, 17, 24), (300, 17, 520),                          # transpose route
])
def test_linear_dgrad_exact(mnk):
    M, N, K = mnk
    dy = _ints((M, N), -2, 2, "lin dy")
    w = _ints((N, K), -1, 1, "lin w")
    ref = dy @ w
    _assert_exact_ok(dy.abs() @ w.abs())
    dx = ext.linear_dgrad(dy.to(BF).to(DEV), w.to(BF).to(DEV))
    assert dx.dtype == BF and dx.shape == (M, K)
    assert torch.equal(dx.cpu(), _bf16_round(ref))


@pytest.mark.parametrize("M", [1, 33, 1000])   # M=1: 31 slabs add zero
@pytest.mark.parametrize("nk", [(10, 520), (16, 8), (1, 24),  # fixed S=32
                                (17, 24)])                    # GEMM route
def test_linear_wgrad_exact(nk, M):
    N, K = nk
    dy = _ints((M, N), -2, 2, "lin dy")
    x = _ints((M, K), -2, 2, "lin x")
    ref = dy.t() @ x
    _assert_exact_ok(dy.abs().t() @ x.abs())
    dw = ext.linear_wgrad(dy.to(BF).to(DEV), x.to(BF).to(DEV))
    assert dw.dtype == torch.float32 and dw.shape == (N, K)
    assert torch.equal(dw.cpu().double(), ref)


# ---------------------------------------------------------------- col_sum ---

@pytest.mark.parametrize("mc", [
    (1, 8), (3, 8), (1000, 8),
    (50, 2056),                        # two windows, 2048 + 8
    (7, 1032),                         # cpg = 129, one walker
    (1, 10), (1000, 10), (9, 255),     # scalar path
])
def test_col_sum_exact(mc):
    M, C = mc
    x = _ints((M, C), -2, 2, "colsum")
    _assert_exact_ok(x.abs().sum(0))
    cs = ext.col_sum(x.to(BF).to(DEV))
    assert cs.dtype == torch.float32 and cs.shape == (C,)
    assert torch.equal(cs.cpu().double(), x.sum(0))


@pytest.mark.parametrize("nchw", [(3, 16, 5, 7), (2, 10, 3, 3)])
def test_col_sum_nhwc_view_exact(nchw):
    """The conv bias gradient: col_sum over the zero-copy [N*H*W, C] view
    of a channels_last tensor."""
    from ddp_tricks_amd.ops.functional import _nhwc_2d
    x = _ints(nchw, -2, 2, "colsum4d")
    _assert_exact_ok(x.abs().sum(dim=(0, 2, 3)))
    cs = ext.col_sum(_nhwc_2d(_act(x)))
    assert torch.equal(cs.cpu().double(), x.sum(dim=(0, 2, 3)))


# ------------------------------------------------------------ elementwise ---

# around the 16 Ki-element block chunk and the 4-wide vector body
MT_SIZES = [1, 3, 4, 5, 16383, 16384, 16385, 2 * 16384 + 3]
# 35 tensors = two launches at MT_MAX = 32; one empty tensor in the middle
MT_SIZES_35 = [((7 * i) % 11) + 1 for i in range(17)] + [0] \
    + [((5 * i) % 13) + 1 for i in range(16)] + [16385]
assert len(MT_SIZES_35) == 35


def _sgd_mirror(p, g, buf, lr, mu, wd, nesterov):
    """float64 mirror of k_mt_sgd:  buf = mu*buf + g ; d = nesterov ?
    g + mu*buf : buf ; p -= lr*d  (g includes wd*p).  Every operand here is
    a small dyadic rational, so float64 AND the kernel's fp32 are exact."""
    gi = g + wd * p if wd != 0 else g
    d = gi
    if mu != 0:
        buf = mu * buf + gi
        d = gi + mu * buf if nesterov != 0 else buf
    return p - lr * d, buf


def _run_sgd(sizes, mu, wd, nesterov, steps=3):
    lr = 0.5
    p64 = [_ints((n,), -4, 4, "p", i) for i, n in enumerate(sizes)]
    b64 = [_ints((n,), -2, 2, "buf", i) for i, n in enumerate(sizes)]
    p = [t.float().to(DEV) for t in p64]
    bufs = [t.float().to(DEV) for t in b64] if mu != 0 else []
    for step in range(steps):
        g64 = [_ints((n,), -3, 3, "g", i, step) for i, n in enumerate(sizes)]
        ext.fused_sgd(p, [t.float().to(DEV) for t in g64], bufs, lr, mu, wd,
                      float(nesterov), None)
        for i in range(len(sizes)):
            p64[i], b64[i] = _sgd_mirror(p64[i], g64[i], b64[i], lr, mu, wd,
                                         nesterov)
            # the mirror itself must be exactly representable in fp32
            assert torch.equal(p64[i].float().double(), p64[i])
    for i in range(len(sizes)):
        assert torch.equal(p[i].cpu().double(), p64[i]), (i, sizes[i])
        if mu != 0:
            assert torch.equal(bufs[i].cpu().double(), b64[i]), (i, sizes[i])


@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("wd", [0.0, 0.25])
@pytest.mark.parametrize("mu", [0.0, 0.5])
def test_fused_sgd_exact(mu, wd, nesterov):
    _run_sgd(MT_SIZES, mu, wd, nesterov)


def test_fused_sgd_two_launches_with_empty_tensor():
    _run_sgd(MT_SIZES_35, 0.5, 0.25, 1)


def test_fused_sgd_flag_set_leaves_p_and_buf():
    p64 = [_ints((n,), -4, 4, "p", i) for i, n in enumerate(MT_SIZES)]
    b64 = [_ints((n,), -2, 2, "buf", i) for i, n in enumerate(MT_SIZES)]
    p = [t.float().to(DEV) for t in p64]
    bufs = [t.float().to(DEV) for t in b64]
    g = [_nonzero_ints((n,), 3, "g", i).float().to(DEV)
         for i, n in enumerate(MT_SIZES)]
    flag = torch.ones(1, device=DEV)
    ext.fused_sgd(p, g, bufs, 0.5, 0.5, 0.25, 1.0, flag)
    for i in range(len(MT_SIZES)):
        assert torch.equal(p[i].cpu().double(), p64[i])
        assert torch.equal(bufs[i].cpu().double(), b64[i])
    assert flag.item() == 1.0


@pytest.mark.parametrize("sizes", [MT_SIZES, MT_SIZES_35])
def test_fused_lookahead_exact(sizes):
    """slow += alpha*(fast - slow); fast = slow — exact at alpha = 0.5."""
    f64 = [_ints((n,), -4, 4, "fast", i) for i, n in enumerate(sizes)]
    s64 = [_ints((n,), -4, 4, "slow", i) for i, n in enumerate(sizes)]
    fast = [t.float().to(DEV) for t in f64]
    slow = [t.float().to(DEV) for t in s64]
    for step in range(3):
        ext.fused_lookahead(fast, slow, 0.5, None)
        for i, n in enumerate(sizes):
            s64[i] = s64[i] + 0.5 * (f64[i] - s64[i])
            f64[i] = s64[i].clone()
            assert torch.equal(slow[i].cpu().double(), s64[i]), (i, n, step)
            assert torch.equal(fast[i].cpu().double(), f64[i]), (i, n, step)
            # move the fast weights apart again, by integers
            d = _ints((n,), -3, 3, "drift", i, step)
            f64[i] = f64[i] + d
            fast[i].add_(d.float().to(DEV))


def test_fused_lookahead_flag_set_changes_nothing():
    f64 = [_ints((n,), -4, 4, "fast", i) for i, n in enumerate(MT_SIZES)]
    s64 = [f + _nonzero_ints(f.shape, 3, "gap", i)
           for i, f in enumerate(f64)]
    fast = [t.float().to(DEV) for t in f64]
    slow = [t.float().to(DEV) for t in s64]
    flag = torch.ones(1, device=DEV)
    ext.fused_lookahead(fast, slow, 0.5, flag)
    for i in range(len(MT_SIZES)):
        assert torch.equal(fast[i].cpu().double(), f64[i])
        assert torch.equal(slow[i].cpu().double(), s64[i])


@pytest.mark.parametrize("sizes", [MT_SIZES, MT_SIZES_35])
def test_multi_tensor_unscale_exact(sizes):
    g64 = [_ints((n,), -8, 8, "unscale", i) for i, n in enumerate(sizes)]
    g = [t.float().to(DEV) for t in g64]
    flag = torch.zeros(1, device=DEV)
    ext.multi_tensor_unscale(g, flag, 0.25)
    for i in range(len(sizes)):
        assert torch.equal(g[i].cpu().double(), g64[i] * 0.25), (i, sizes[i])
    assert flag.item() == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", [
    (5, 4),              # last element of a scalar tail
    (16385, 16384),      # a one-element tail in the second chunk
    (16385, 1001),       # inside a vector body
])
def test_multi_tensor_unscale_sets_flag(where, bad):
    n, idx = where
    g64 = _ints((n,), -8, 8, "unscale bad")
    g = g64.float().to(DEV)
    g[idx] = bad
    flag = torch.zeros(1, device=DEV)
    ext.multi_tensor_unscale([g], flag, 0.25)
    assert flag.item() == 1.0
    # every other element is still scaled exactly
    keep = torch.ones(n, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(g.cpu().double()[keep], (g64 * 0.25)[keep])
    # a clean call leaves an already-set flag set
    clean = _ints((n,), -8, 8, "unscale clean").float().to(DEV)
    ext.multi_tensor_unscale([clean], flag, 0.25)
    assert flag.item() == 1.0


@pytest.mark.parametrize("C", [1, 3, 7])
def test_pad8_channels_exact(C):
    x = _ints((2, C, 5, 7), -2, 2, "pad8")
    want = torch.zeros(2, 8, 5, 7, dtype=BF)
    want[:, :C] = x.to(BF)
    xp = ext.pad8_channels(_act(x))
    assert xp.shape == (2, 8, 5, 7) and xp.dtype == BF
    assert xp.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(xp.cpu(), want)


@pytest.mark.parametrize("numel", [1, 7, 8, 4099])
def test_cast_to_bf16_exact(numel):
    """Bit-equal to torch's round-to-nearest-even cast, with rounding
    ties (odd integers in 256..512 and integers = 2 mod 4 in 512..1024
    sit half-way between bf16 values; both the round-up and the
    round-down-to-even kind occur), +-inf and +-0."""
    g = torch.Generator().manual_seed(_seed("cast", numel))
    x = torch.randn(numel, generator=g) * 100.0
    i = torch.arange(numel)
    ties = torch.where(i % 2 == 0, 257 + 2 * (i % 128),
                       514 + 4 * (i % 127)).float()
    sel = i % 3 != 2
    x[sel] = ties[sel]
    if numel >= 7:
        x[1] = float("inf")
        x[2] = float("-inf")
        x[3] = 0.0
        x[4] = -0.0
        x[5] = 259.0          # tie, rounds up to even mantissa (260)
        x[6] = 257.0          # tie, rounds down to even mantissa (256)
    want = x.to(BF)
    y = ext.cast_to_bf16(x.to(DEV))
    assert y.dtype == BF and y.shape == x.shape
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("nchw", [
    (3, 24, 1, 1),       # HW = 1
    (2, 300, 8, 8),      # HW = 64 (vector path), two channel blocks
    (17, 40, 3, 5),      # HW = 15: scalar path
])
def test_nhwc_unflatten_exact(nchw):
    N, C, H, W = nchw
    dy = _ints((N, C * H * W), -128, 128, "unflatten").to(BF)
    dx = ext.nhwc_unflatten(dy.to(DEV), C, H, W)
    assert dx.shape == (N, C, H, W)
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(dx.cpu(), dy.view(N, C, H, W))
    # and it inverts nhwc_flatten
    assert torch.equal(ext.nhwc_flatten(dx).cpu(), dy)


# ------------------------------------------------------- input validation ---

def test_hip_conv2d_refuses_non_uniform_padding():
    """The HIP kernels take one stride and one padding: a non-uniform
    tuple must raise, never silently compute with its first element."""
    from ddp_tricks_amd.ops.modules import Conv2d
    conv = Conv2d(8, 8, (1, 3), padding=(0, 1)).to(DEV)
    x = _act(_ints((2, 8, 5, 7), -2, 2, "val x"))
    with pytest.raises(ValueError):
        conv(x)
    conv2 = Conv2d(8, 8, 3, stride=(1, 2), padding=1).to(DEV)
    with pytest.raises(ValueError):
        conv2(x)
