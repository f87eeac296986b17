"""k_gemm_dma (gemm.hip): the LDS-DMA GEMM of the linear layers.

* Bit-identity: impl=1 against impl=0 by ``torch.equal`` on random bf16 data,
  for gemm_tn, linear_fwd, linear_act_fwd (ReLU and dropout), linear_dgrad
  and linear_wgrad.  ``linear_plan`` is asserted first, so no case compares
  the legacy kernel with itself.
* Exact data: small integers against a float64 product with equality (the
  idiom of test_gpu_exact.py), so a wrong swizzle or transposed read fails
  without the legacy kernel as witness.
* Tails: operands are row slices of NaN-filled buffers, so a read past M, N
  or a split's K end turns an output into NaN.
* Plan, and one autograd step at Linear(8192 -> 512)'s shape.

The edge set is given in GEMM terms, C[gm, gn] contracting gk: gm and gn in
{8, 120, 128, 136, 264} (below a tile, a tile, a tile and a tail, three
tiles), gk in {64, 72, 128, 200, 1024} (72 and 200 end a split inside a
K-tile, 1024 splits 16 ways at one tile and 4 to 16 ways elsewhere); the full
product runs, (264, 264, 1024) being the case with several tiles in both
grid dimensions and a split.  Each entry point maps its own (M, N, K) onto
those: forward and gemm_tn (M, N, K) = (gm, gn, gk), dgrad (gm, gk, gn),
wgrad (gk, gm, gn).  A linear layer with N <= 16 belongs to the small
kernels: such cases assert the plan says so and are reached through gemm_tn.
"""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

from test_gpu_exact import _assert_exact_ok, _bf16_round, _ints

BF = torch.bfloat16
FWD, DGRAD, WGRAD, GEMM = 0, 1, 2, 3
MN_EDGES = (8, 120, 128, 136, 264)
K_EDGES = (64, 72, 128, 200, 1024)
SEED = 0x5DEECE66D
THR, SCALE = 16384, 65536.0 / (65536.0 - 16384.0)

# what the automatic plan routes (docs/KERNELS.md, "Linear GEMM: LDS-DMA
# tiles", benchmark table): Toy_Net's Linear(8192, 512) at B = 1024, VGG-16's
# Linear(25088, 4096) and Linear(4096, 4096) at B = 256
ROUTED = {FWD: "dma", DGRAD: "dma", WGRAD: "dma"}
BENCH_SHAPES = [(1024, 512, 8192), (256, 4096, 25088), (256, 4096, 4096)]


def _poisoned(rows, cols, gen, ints=False):
    """[rows, cols] bf16 values as a slice of a NaN-filled buffer, three NaN
    rows in front and three behind."""
    buf = torch.full((rows + 6, cols), float("nan"), dtype=BF, device=DEV)
    if ints:
        v = torch.randint(-2, 3, (rows, cols), generator=gen, device=DEV)
    else:
        v = torch.randn(rows, cols, generator=gen, device=DEV)
    buf[3:3 + rows] = v.to(BF)
    out = buf[3:3 + rows]
    # 16-byte aligned, or the entry point would keep it off the DMA kernel
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return out


@functools.lru_cache(maxsize=None)
def _operands(gm, gn, gk):
    """Random bf16 A [gm, gk], B [gn, gk], dgrad's B [gk, gn], wgrad's
    operands [gk, gm] and [gk, gn], all inside NaN, and an fp32 bias."""
    g = torch.Generator(device=DEV).manual_seed(gm * 1000003 + gn * 1009 + gk)
    return dict(a=_poisoned(gm, gk, g), b=_poisoned(gn, gk, g),
                b_km=_poisoned(gk, gn, g), a_km=_poisoned(gk, gm, g),
                bias=torch.randn(gn, generator=g, device=DEV))


def _same(a, b, tag):
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    assert not torch.isnan(b.float()).any(), tag
    # bit patterns, so a -0 / +0 or NaN-payload difference also counts
    bits = torch.int16 if a.dtype == BF else torch.int32
    assert torch.equal(a.view(bits), b.view(bits)), tag


@pytest.mark.parametrize("gk", K_EDGES)
def test_bit_identical_to_legacy(gk):
    for gm, gn in itertools.product(MN_EDGES, MN_EDGES):
        o = _operands(gm, gn, gk)
        tag = (gm, gn, gk)
        # gemm_tn: bf16 and fp32 output, bias on and off
        assert ext.linear_plan(GEMM, gm, gn, gk, 1) == "dma"
        assert ext.linear_plan(GEMM, gm, gn, gk, 0) == "legacy"
        for out_f32, bias in itertools.product((False, True),
                                               (None, o["bias"])):
            _same(ext.gemm_tn(o["a"], o["b"], bias, out_f32, 0),
                  ext.gemm_tn(o["a"], o["b"], bias, out_f32, 1),
                  ("gemm_tn", tag, out_f32, bias is not None))
        # forward entry points (N <= 16: the small kernels, not this one)
        if gn <= 16:
            assert ext.linear_plan(FWD, gm, gn, gk, 1) == "legacy"
        else:
            assert ext.linear_plan(FWD, gm, gn, gk, 1) == "dma"
            for bias in (None, o["bias"]):
                _same(ext.linear_fwd(o["a"], o["b"], bias, 0),
                      ext.linear_fwd(o["a"], o["b"], bias, 1),
                      ("linear_fwd", tag, bias is not None))
                for thr, scale in ((0, 1.0), (THR, SCALE)):
                    _same(ext.linear_act_fwd(o["a"], o["b"], bias, thr,
                                             scale, SEED, 0),
                          ext.linear_act_fwd(o["a"], o["b"], bias, thr,
                                             scale, SEED, 1),
                          ("linear_act_fwd", tag, bias is not None, thr))
        # dgrad: dy [M, N] = a, w [N, K] = b_km with (M, N, K) = (gm, gk, gn)
        if gk <= 16:
            assert ext.linear_plan(DGRAD, gm, gk, gn, 1) == "legacy"
        else:
            assert ext.linear_plan(DGRAD, gm, gk, gn, 1) == "dma"
            _same(ext.linear_dgrad(o["a"], o["b_km"], 0),
                  ext.linear_dgrad(o["a"], o["b_km"], 1), ("dgrad", tag))
        # wgrad: dy [M, N] = a_km, x [M, K] = b_km, (M, N, K) = (gk, gm, gn)
        if gm <= 16:
            assert ext.linear_plan(WGRAD, gk, gm, gn, 1) == "legacy"
        else:
            assert ext.linear_plan(WGRAD, gk, gm, gn, 1) == "dma"
            _same(ext.linear_wgrad(o["a_km"], o["b_km"], 0),
                  ext.linear_wgrad(o["a_km"], o["b_km"], 1), ("wgrad", tag))


@pytest.mark.parametrize("gk", K_EDGES)
def test_exact_against_float64(gk):
    """Integers in [-2, 2]: every sum is below 2 * 2 * 1024 + 400, exact in
    fp32 in any order.  Operands sit inside NaN here too."""
    for gm, gn in itertools.product(MN_EDGES, MN_EDGES):
        g = torch.Generator(device=DEV).manual_seed(gm * 7919 + gn * 31 + gk)
        a = _poisoned(gm, gk, g, ints=True)
        b = _poisoned(gn, gk, g, ints=True)
        b_km = _poisoned(gk, gn, g, ints=True)
        a_km = _poisoned(gk, gm, g, ints=True)
        bias = _ints((gn,), -400, 400, "dma bias")
        a64, b64 = a.cpu().double(), b.cpu().double()
        bk64, ak64 = b_km.cpu().double(), a_km.cpu().double()
        tag = (gm, gn, gk)
        ref = a64 @ b64.t()
        _assert_exact_ok(a64.abs() @ b64.abs().t() + bias.abs())
        assert ext.linear_plan(GEMM, gm, gn, gk, 1) == "dma"
        got = ext.gemm_tn(a, b, None, True, 1)
        assert torch.equal(got.cpu().double(), ref), ("gemm f32", tag)
        got = ext.gemm_tn(a, b, bias.float().to(DEV), True, 1)
        assert torch.equal(got.cpu().double(), ref + bias), ("gemm f32 b", tag)
        got = ext.gemm_tn(a, b, bias.float().to(DEV), False, 1)
        assert torch.equal(got.cpu(), _bf16_round(ref + bias)), ("gemm", tag)
        if gn > 16:
            got = ext.linear_act_fwd(a, b, bias.float().to(DEV), 0, 1.0,
                                     SEED, 1)
            assert torch.equal(got.cpu(),
                               _bf16_round(torch.relu(ref + bias))), tag
        if gk > 16:
            ref_dx = a64 @ bk64
            _assert_exact_ok(a64.abs() @ bk64.abs())
            got = ext.linear_dgrad(a, b_km, 1)
            assert torch.equal(got.cpu(), _bf16_round(ref_dx)), ("dgrad", tag)
        if gm > 16:
            ref_dw = ak64.t() @ bk64
            _assert_exact_ok(ak64.abs().t() @ bk64.abs())
            got = ext.linear_wgrad(a_km, b_km, 1)
            assert got.dtype == torch.float32
            assert torch.equal(got.cpu().double(), ref_dw), ("wgrad", tag)


def test_dropout_mask_is_the_formula():
    """The mask depends on row * N + col alone: the fused output at p = 0.25
    is the ReLU output scaled or zeroed by functional.dropout_mask."""
    from ddp_tricks_amd.ops.functional import dropout_mask
    M, N, K = 136, 264, 200
    o = _operands(M, N, K)
    assert ext.linear_plan(FWD, M, N, K, 1) == "dma"
    relu = ext.linear_act_fwd(o["a"], o["b"], o["bias"], 0, 1.0, SEED, 1)
    drop = ext.linear_act_fwd(o["a"], o["b"], o["bias"], THR, SCALE, SEED, 1)
    keep = torch.from_numpy(dropout_mask(SEED, M * N, THR)).view(M, N)
    kept = drop.cpu().float() != 0
    assert not (kept & ~keep).any()
    assert torch.equal(kept, keep & (relu.cpu().float() > 0))


@pytest.mark.parametrize("mnk", [(100, 70, 130),   # nothing a multiple of 8
                                 (128, 128, 68),   # K % 8 != 0 alone
                                 (128, 132, 64)])  # N % 8 != 0 alone
def test_misfit_plans_legacy_and_is_exact(mnk):
    M, N, K = mnk
    for op in (FWD, DGRAD, WGRAD, GEMM):
        for impl in (-1, 0, 1):
            assert ext.linear_plan(op, M, N, K, impl) == "legacy"
    x = _ints((M, K), -2, 2, "misfit x")
    w = _ints((N, K), -1, 1, "misfit w")
    dy = _ints((M, N), -2, 2, "misfit dy")
    _assert_exact_ok(x.abs() @ w.abs().t())
    xd, wd, dyd = (t.to(BF).to(DEV) for t in (x, w, dy))
    assert torch.equal(ext.linear_fwd(xd, wd, None, 1).cpu(),
                       _bf16_round(x @ w.t()))
    assert torch.equal(ext.linear_dgrad(dyd, wd, 1).cpu(),
                       _bf16_round(dy @ w))
    assert torch.equal(ext.linear_wgrad(dyd, xd, 1).cpu().double(),
                       dy.t() @ x)


def test_plan():
    # a bad impl raises, from the plan and from every entry point
    o = _operands(128, 128, 64)
    for bad in (-2, 2):
        with pytest.raises(RuntimeError):
            ext.linear_plan(FWD, 128, 128, 64, bad)
        with pytest.raises(RuntimeError):
            ext.linear_fwd(o["a"], o["b"], None, bad)
        with pytest.raises(RuntimeError):
            ext.linear_act_fwd(o["a"], o["b"], None, 0, 1.0, SEED, bad)
        with pytest.raises(RuntimeError):
            ext.linear_dgrad(o["a"], o["b_km"], bad)
        with pytest.raises(RuntimeError):
            ext.linear_wgrad(o["a_km"], o["b_km"], bad)
        with pytest.raises(RuntimeError):
            ext.gemm_tn(o["a"], o["b"], None, False, bad)
    with pytest.raises(RuntimeError):
        ext.linear_plan(4, 128, 128, 64, -1)
    # the 10-class head stays with the small kernels, forced or not
    for op in (FWD, DGRAD, WGRAD):
        for impl in (-1, 0, 1):
            assert ext.linear_plan(op, 1024, 10, 512, impl) == "legacy"
            assert ext.linear_plan(op, 1024, 16, 512, impl) == "legacy"
    # the benchmarked shapes follow the routing table
    for M, N, K in BENCH_SHAPES:
        for op in (FWD, DGRAD, WGRAD):
            assert ext.linear_plan(op, M, N, K) == ROUTED[op], (op, M, N, K)
            assert ext.linear_plan(op, M, N, K, 0) == "legacy"
            assert ext.linear_plan(op, M, N, K, 1) == "dma"


def test_small_head_unchanged_by_impl():
    M, N, K = 33, 10, 520
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, generator=g, device=DEV).to(BF)
    w = torch.randn(N, K, generator=g, device=DEV).to(BF)
    dy = torch.randn(M, N, generator=g, device=DEV).to(BF)
    for impl in (0, 1):
        assert torch.equal(ext.linear_fwd(x, w, None, impl),
                           ext.linear_fwd(x, w, None))
        assert torch.equal(ext.linear_dgrad(dy, w, impl),
                           ext.linear_dgrad(dy, w))
        assert torch.equal(ext.linear_wgrad(dy, x, impl),
                           ext.linear_wgrad(dy, x))


def test_autograd_step_matches_legacy_entry_points():
    """One Linear(8192 -> 512) step at B = 8 through ops.functional.linear
    under the automatic plan, against the impl=0 entry points."""
    from ddp_tricks_amd.ops.functional import linear
    M, N, K = 8, 512, 8192
    for op in (FWD, DGRAD, WGRAD):
        assert ext.linear_plan(op, M, N, K) == ROUTED[op]
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(M, K, generator=g, device=DEV).to(BF).requires_grad_(True)
    w = (torch.randn(N, K, generator=g, device=DEV) / 64).requires_grad_(True)
    b = torch.randn(N, generator=g, device=DEV).requires_grad_(True)
    dy = torch.randn(M, N, generator=g, device=DEV).to(BF)
    y = linear(x, w, b)
    y.backward(dy)
    xb, wb = x.detach(), w.detach().to(BF)
    _same(ext.linear_fwd(xb, wb, b.detach(), 0), y.detach(), "y")
    _same(ext.linear_dgrad(dy, wb, 0), x.grad, "dx")
    _same(ext.linear_wgrad(dy, xb, 0), w.grad, "dw")
    _same(ext.col_sum(dy), b.grad, "db")
