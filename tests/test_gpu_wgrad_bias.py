"""conv2d_wgrad_bias: the bias gradient produced inside the wgrad launches,
and the streaming stem (C = 1, 3x3) wgrad kernel.

Three tiers, all @pytest.mark.gpu:

* exact — integer inputs as in test_gpu_exact.py (dy, x in {-2..2}); while
  the sum of |terms| stays below 2^24 (asserted on the float64 reference
  alone) fp32 accumulation is exact in any order, so dw and db are compared
  with ``torch.equal``;
* random bf16 data — dw of the MFMA leaves must be bit-equal to
  conv2d_wgrad; db and the stem kernel's dw are compared element-wise with a
  float64 reference under the rigorous bound |err| <= gamma * sum|terms|,
  gamma = (L + T) * 2^-24 (derivation below); two calls give equal bits;
* autograd — functional.conv2d with bias against the DDPX_WGRAD_BIAS=0 path.

The bound.  Every dy*x product of two bf16 values is exact in fp32 (16
significand bits) and each fmaf / add rounds once, relative error <= u =
2^-24.  A term that passes through n roundings on its way to the output
carries a factor within (1 +- u)^n, so |err| <= ((1+u)^n - 1) * sum|terms|.
L + T below counts every addition on the longest path INCLUDING the first
addition into a zero accumulator of each stage, which is exact; with at
least two such exact steps counted, (n-2)u / (1 - (n-2)u) <= n*u for all
n < 5792, so gamma = (L + T) * u is rigorous for the sizes used here.

  streaming stem kernel (k_wgrad_c1_r3_stream), as the host sizes it:
    rpl = 64 // (Ko/8) rows per wave load, nloads = ceil(M / rpl),
    S = clamp(ceil(nloads / 32), 1, 768) blocks, each wave owns
    ceil(nloads / 4S) loads and a lane takes one row of each:
      L = ceil(nloads / (4*S))             serial fmaf chain per lane
      T = 4*rpl                            LDS sum of 4 waves x rpl rows
        + ceil(S/64) + 6                   combine: lane sweep + 6 shuffles
  wide_pair<DEPTH> bias, which wide_dma<DEPTH>'s chain stays inside (DEPTH
  32 for Kgemm < 1152, else 64), split S from the host's loop counted with
  DEPTH (see _wide_pair_gamma for where the host's own S is smaller):
      L = ceil(ceil(M/DEPTH) / S) * DEPTH/2   half-row chain per thread
        + 1                                    the other half (shuffle)
      T = S                 if S <= 16         one serial combine
        = 4 + 1 + S/8       otherwise          two 4-chains, their sum,
                                               then S/8 chunks serially
"""
import functools
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

BF = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)
U = 2.0 ** -24


# ---------------------------------------------------------------- helpers ---

def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(shape, lo, hi, *key):
    g = torch.Generator().manual_seed(_seed(shape, lo, hi, *key))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _randn_bf16(shape, *key):
    """float64 CPU tensor of bf16-representable normal values."""
    g = torch.Generator().manual_seed(_seed(shape, *key))
    return torch.randn(tuple(shape), generator=g).to(BF).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _act(t64):
    return _nhwc(t64.to(BF)).to(DEV)


def _out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _cdiv(a, b):
    return -(-a // b)


def _stem_gamma(M, Ko):
    rpl = 64 // (Ko // 8)
    nloads = _cdiv(M, rpl)
    S = max(1, min(768, _cdiv(nloads, 32)))
    L = _cdiv(nloads, 4 * S)
    T = 4 * rpl + _cdiv(S, 64) + 6
    return (L + T) * U


def _wide_pair_gamma(M, Ko, Kgemm, count_depth=None):
    """(gamma, S).  The host's split loop counts contraction steps 64 deep on
    every wide leaf; ``count_depth=64`` gives that S, which the plan tests
    below hold equal to conv2d_wgrad_plan's.  The default counts with the
    leaf's own depth as this file always has: on a 32-deep row whose M ends
    the loop it doubles once more, and that larger S makes gamma SMALLER
    than the rigorous one (154u against 289u at M = 8320), so the bound
    checks keep using it: they ask more, not less."""
    assert Ko >= 128 and Kgemm >= 128
    depth = 64 if Kgemm >= 1152 else 32
    tiles = _cdiv(Ko, 128) * _cdiv(Kgemm, 128)
    assert tiles >= 8 or M >= 262144, "shape does not reach wide_pair"
    S = 1
    while (tiles * S < 1024 and S < 512
           and M // (S * 2 * (count_depth or depth)) >= 8):
        S *= 2
    L = _cdiv(_cdiv(M, depth), S) * (depth // 2) + 1
    T = S if S <= 16 else 4 + 1 + _cdiv(S, 8)
    return (L + T) * U, S


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Inputs and float64 references, computed once per (shape, kind) and
    shared read-only: (x, dy, dw_ref, dw_abs, db_ref, db_abs)."""
    N, C, H, W, K, R, S, stride, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    if kind == "int":
        x = _ints((N, C, H, W), -2, 2, "x")
        dy = _ints((N, K, P, Q), -2, 2, "dy")
    else:
        x = _randn_bf16((N, C, H, W), "x")
        dy = _randn_bf16((N, K, P, Q), "dy")
    dw = torch.nn.grad.conv2d_weight(x, (K, C, R, S), dy, stride=stride,
                                     padding=pad)
    dw_abs = torch.nn.grad.conv2d_weight(x.abs(), (K, C, R, S), dy.abs(),
                                         stride=stride, padding=pad)
    return x, dy, dw, dw_abs, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


# shapes (N, C, H, W, K, R, S, stride, pad), each with the leaf name that
# conv2d_wgrad_plan must report for it (test_rows_reach_the_leaf_they_name)
_LEAF_ROWS = [
    ((2, 8, 5, 7, 8, 3, 3, 1, 1), "sb_pair<64>"),      # S_ = 1
    ((4, 8, 64, 65, 8, 1, 1, 1, 0), "sb_pair<64>"),    # two-stage combine
    ((2, 8, 6, 6, 72, 3, 3, 1, 1), "sb_pair<32>"),     # gk = 2
    ((2, 56, 6, 5, 136, 3, 3, 1, 1), "wide_dma<32>"),  # Ko, Kgemm=504 tails
    ((2, 128, 5, 6, 128, 3, 3, 1, 1), "wide_dma<64>"),   # Kgemm = 1152
    ((2, 136, 5, 6, 136, 3, 3, 1, 1), "wide_dma<64>"),   # with tails
    ((2, 16, 10, 13, 32, 3, 3, 3, 1), "sb_pair<64>"),  # stride 3
    ((2, 8, 12, 10, 64, 3, 1, 2, 0), "sb_pair<64>"),   # R != S
    ((1, 1, 3, 3, 8, 3, 3, 1, 0), "c1_r3_stream"),     # M = 1, Ko = 8
    ((3, 1, 7, 9, 8, 3, 3, 1, 1), "c1_r3_stream"),     # padded
    ((3, 1, 9, 8, 16, 3, 3, 2, 0), "c1_r3_stream"),    # stride 2
    ((2, 3, 6, 8, 16, 2, 2, 1, 0), "small_rsc"),       # rsc = 12
    ((2, 1, 7, 6, 8, 4, 4, 1, 1), "small_rsc"),        # rsc = 16
    ((2, 3, 7, 6, 16, 3, 3, 1, 1), "small_cin"),       # rsc = 27
    ((2, 1, 6, 7, 72, 3, 3, 1, 1), "small_cin"),       # Ko > 64
    ((2, 3, 7, 6, 136, 3, 3, 1, 0), "small_cin"),      # Ko > 64
    ((2, 1, 5, 6, 12, 3, 3, 1, 1), "c1_r3"),           # Ko % 8 != 0
    ((4, 128, 64, 65, 128, 1, 1, 1, 0), "sb_pair<32>"),  # M = 16640, split
                        # > 16, two-stage combine, M % (split*depth) != 0
]
LEAF_SHAPES = [shape for shape, _ in _LEAF_ROWS]
# rows whose purpose is the two-stage combine: the plan's split must be > 16
TWO_STAGE_SB_SHAPES = [LEAF_SHAPES[1], LEAF_SHAPES[17]]
# fused-bias leaves at deep splits, M no multiple of split * depth.  The
# host's split is 16 on the first row (it counts 64 deep, see
# _wide_pair_gamma): the deepest ONE-stage combine.  On the other two it is
# 32: bias partials through BOTH combine kernels, at either depth.
_DEEP_WIDE_ROWS = [
    ((2, 512, 64, 65, 256, 1, 1, 1, 0), "wide_dma<32>"),  # 8 tiles, M = 8320
    ((4, 128, 64, 65, 128, 3, 3, 1, 1), "wide_dma<64>"),  # 9 tiles, M = 16640
    ((16, 56, 33, 32, 136, 3, 3, 1, 1), "wide_dma<32>"),  # 8 tiles, M = 16896
]
DEEP_WIDE_SHAPES = [shape for shape, _ in _DEEP_WIDE_ROWS]
TWO_STAGE_WIDE_SHAPES = DEEP_WIDE_SHAPES[1:]
STEM_SHAPES = [
    (1, 1, 3, 3, 64, 3, 3, 1, 0),     # M = 1
    (3, 1, 7, 9, 64, 3, 3, 1, 1),     # padded; row and image wraps inside
                                      # one 8-row wave load (Q = 9, PQ = 63)
    (5, 1, 28, 28, 64, 3, 3, 1, 0),   # M = 3380: 14 blocks, M % 8 != 0,
                                      # M % chunk != 0
    (5, 1, 28, 28, 8, 3, 3, 1, 0),    # 1 lane per row, 64 rows per load
    (5, 1, 28, 28, 24, 3, 3, 1, 0),   # 3 lanes per row: lane 63 idle
    (5, 1, 28, 28, 56, 3, 3, 1, 0),   # 7 lanes per row: lane 63 idle
    (4, 1, 11, 13, 40, 3, 3, 2, 1),   # stride 2, padded, 5 lanes per row
]
WIDE_PAIR_SHAPES = [
    (2, 56, 6, 5, 136, 3, 3, 1, 1),
    (2, 128, 5, 6, 128, 3, 3, 1, 1),
    (2, 136, 5, 6, 136, 3, 3, 1, 1),
] + DEEP_WIDE_SHAPES


def _m_kgemm(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    return N * P * Q, R * S * C


def test_shape_tables_reach_what_they_claim():
    for shape in DEEP_WIDE_SHAPES:
        M, Kgemm = _m_kgemm(shape)
        _, S = _wide_pair_gamma(M, shape[4], Kgemm)
        depth = 64 if Kgemm >= 1152 else 32
        assert S > 16 and M % (S * depth) != 0
    for shape in WIDE_PAIR_SHAPES:
        _wide_pair_gamma(_m_kgemm(shape)[0], shape[4], _m_kgemm(shape)[1])
    for shape in STEM_SHAPES:
        assert shape[1] == 1 and shape[4] % 8 == 0 and shape[4] <= 64


def _plan(shape, want_bias):
    """(leaf name, split, fused_bias) from the host's own plan function."""
    return ext.conv2d_wgrad_plan(*shape, want_bias)


def test_rows_reach_the_leaf_they_name():
    """Ask the host which leaf and split it launches, instead of guessing."""
    rows = (_LEAF_ROWS + _DEEP_WIDE_ROWS
            + [(shape, "c1_r3_stream") for shape in STEM_SHAPES])
    for shape, leaf in rows:
        fused = leaf.startswith(("wide_", "c1_r3_stream"))
        for want_bias in (False, True):
            got_leaf, _, got_fused = _plan(shape, want_bias)
            assert got_leaf == leaf, (shape, got_leaf)
            assert got_fused == (want_bias and fused), shape
    for shape in TWO_STAGE_SB_SHAPES + TWO_STAGE_WIDE_SHAPES:
        assert _plan(shape, True)[1] > 16, shape
    for shape in TWO_STAGE_WIDE_SHAPES:
        M, Kgemm = _m_kgemm(shape)
        depth = 64 if Kgemm >= 1152 else 32
        assert M % (_plan(shape, True)[1] * depth) != 0
    assert _plan(DEEP_WIDE_SHAPES[0], True)[1] == 16
    for shape in WIDE_PAIR_SHAPES:
        M, Kgemm = _m_kgemm(shape)
        rigorous, S = _wide_pair_gamma(M, shape[4], Kgemm, count_depth=64)
        assert _plan(shape, True)[1] == _plan(shape, False)[1] == S, shape
        # the gamma the bound checks use is never the larger one
        assert _wide_pair_gamma(M, shape[4], Kgemm)[0] <= rigorous


# ------------------------------------------------------------------ exact ---

@pytest.mark.parametrize("shape",
                         LEAF_SHAPES + DEEP_WIDE_SHAPES + STEM_SHAPES)
def test_wgrad_bias_exact(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy, dw_ref, dw_abs, db_ref, db_abs = _case(shape, "int")
    assert dw_abs.max().item() < EXACT_LIMIT
    assert db_abs.max().item() < EXACT_LIMIT
    dw, db = ext.conv2d_wgrad_bias(_act(dy), _act(x), R, S, stride, pad)
    assert dw.dtype == torch.float32 and dw.shape == (K, C, R, S)
    assert db.dtype == torch.float32 and db.shape == (K,)
    assert torch.equal(dw.cpu().double(), dw_ref)
    assert torch.equal(db.cpu().double(), db_ref)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_wgrad_without_bias_exact(shape):
    """conv2d_wgrad dispatches the same shapes to the streaming kernel."""
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy, dw_ref, dw_abs, _, _ = _case(shape, "int")
    assert dw_abs.max().item() < EXACT_LIMIT
    dw = ext.conv2d_wgrad(_act(dy), _act(x), R, S, stride, pad)
    assert torch.equal(dw.cpu().double(), dw_ref)


# ------------------------------------------------------- random bf16 data ---

def _assert_within(got, ref, abs_sum, gamma, what):
    err = (got.cpu().double() - ref).abs()
    bound = gamma * abs_sum
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}, gamma {gamma:.3e}")
    assert worst <= 0.0, (what, worst)


@pytest.mark.parametrize("shape", WIDE_PAIR_SHAPES)
def test_wide_pair_random(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy, _, _, db_ref, db_abs = _case(shape, "rand")
    M, Kgemm = _m_kgemm(shape)
    gamma, _ = _wide_pair_gamma(M, K, Kgemm)
    dyd, xd = _act(dy), _act(x)
    dw_plain = ext.conv2d_wgrad(dyd, xd, R, S, stride, pad)
    dw, db = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
    assert torch.equal(dw, dw_plain)
    _assert_within(db, db_ref, db_abs, gamma, "db")
    dw2, db2 = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_random(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy, dw_ref, dw_abs, db_ref, db_abs = _case(shape, "rand")
    M, _ = _m_kgemm(shape)
    gamma = _stem_gamma(M, K)
    dyd, xd = _act(dy), _act(x)
    dw, db = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
    _assert_within(dw, dw_ref, dw_abs, gamma, "dw")
    _assert_within(db, db_ref, db_abs, gamma, "db")
    dw_plain = ext.conv2d_wgrad(dyd, xd, R, S, stride, pad)
    _assert_within(dw_plain, dw_ref, dw_abs, gamma, "dw (no bias)")
    dw2, db2 = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.equal(dw_plain, ext.conv2d_wgrad(dyd, xd, R, S, stride, pad))


# --------------------------------------------------------------- autograd ---

def _autograd_grads(shape, x, w, b, dy):
    from ddp_tricks_amd.ops import functional as F_ops
    N, C, H, W, K, R, S, stride, pad = shape
    xd = _act(x)
    wd = torch.nn.Parameter(w.float().to(DEV))
    bd = torch.nn.Parameter(b.float().to(DEV))
    y = F_ops.conv2d(xd, wd, bd, stride=stride, padding=pad)
    y.backward(_act(dy).to(y.dtype))
    return wd.grad.detach().clone(), bd.grad.detach().clone()


@pytest.mark.parametrize("shape,mfma", [
    ((2, 56, 6, 5, 136, 3, 3, 1, 1), True),     # wide_dma<32>
    ((5, 1, 28, 28, 64, 3, 3, 1, 0), False),    # streaming stem kernel
])
def test_autograd_matches_col_sum_path(shape, mfma, monkeypatch):
    """Fused path against DDPX_WGRAD_BIAS=0.  dw: bit-equal on the MFMA
    leaf; on the stem both are held to the kernel's bound against float64.
    db: the col_sum oracle sums M terms in SOME order, so any term passes
    at most M roundings: |fused - oracle| <= (gamma + M*u) * sum|dy|."""
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy, dw_ref, dw_abs, db_ref, db_abs = _case(shape, "rand")
    w = _randn_bf16((K, C, R, S), "w")
    b = _randn_bf16((K,), "b")
    M, Kgemm = _m_kgemm(shape)
    gamma = (_wide_pair_gamma(M, K, Kgemm)[0] if mfma
             else _stem_gamma(M, K))
    monkeypatch.setenv("DDPX_WGRAD_BIAS", "1")
    dw_f, db_f = _autograd_grads(shape, x, w, b, dy)
    monkeypatch.setenv("DDPX_WGRAD_BIAS", "0")
    dw_o, db_o = _autograd_grads(shape, x, w, b, dy)
    assert dw_f.shape == (K, C, R, S) and db_f.shape == (K,)
    if mfma:
        assert torch.equal(dw_f, dw_o)
    else:
        _assert_within(dw_f, dw_ref, dw_abs, gamma, "dw fused")
        _assert_within(dw_o, dw_ref, dw_abs, gamma, "dw oracle")
    _assert_within(db_f, db_ref, db_abs, gamma, "db fused")
    _assert_within(db_f, db_o.cpu().double(), db_abs, gamma + M * U,
                   "db fused vs col_sum")
