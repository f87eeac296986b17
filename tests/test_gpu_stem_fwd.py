"""Direct C = 1 3x3 stem forward (conv.hip, k_conv_c1_r3_fwd) against the
MFMA path on zero-padded channels and against float64.  All tests
@pytest.mark.gpu (the plan binding needs the extension, which links the
device runtime).

Notation: u = 2^-24 (fp32 unit roundoff), x and w are the bf16-rounded
operands, v = sum_k x_k w_k + b is the pre-rounding value, y = bf16(v).

* Plan: conv2d_stem_plan is pure arithmetic on the shape.
* Exact data: x in {-2..2}, w in {-1, -1/2, 0, 1/2, 1}, b in {-3..3}.  Every
  product is a multiple of 1/2 below 2, every partial sum a multiple of 1/2
  below 32: exact in fp32 whatever the order, and |v| <= 21 with one
  fractional bit is exact in bf16.  v^2 <= 441 has two fractional bits and
  the per-channel totals stay below 2^22 (asserted on the float64
  reference), so every statistics addition is exact too.  Both paths must
  then give the same y (``torch.equal``) and the same per-channel totals;
  the slabs have different widths, so each is summed in float64 first.
* Random data: the kernel forms nine exact products (8 x 8 significand
  bits) and adds them with at most nine roundings, bias included (the first
  product enters an accumulator of 0 exactly): |v - v64| <= e = 10 u A with
  A = sum|x w| + |b|.  y = RNE_bf16(v) adds half a bf16 ulp of v.  bf16 has
  8 significand bits, so half an ulp of a value in [2^k, 2^(k+1)) is
  2^(k-8): between 2^-9 |v| (top of the binade) and 2^-8 |v| (bottom).  The
  bound asserted is
      |y - v64| <= hulp(|v64| + e) + e,     hulp(t) = 2^(floor(log2 t) - 8),
  the least a correctly rounded result can be held to.  The issue writes
  the first term as 2^-9 |v64|, which is the half-ulp only at the top of a
  binade; no RNE bf16 result meets that elsewhere (measured on this kernel:
  max |y - v64| / (2^-9 |v64| + e) = 1.93 to 1.99 over the shapes here, and
  the MFMA path gives the same figure), so the half-ulp itself is used.
  Both ratios are printed.
* Random statistics: a lane adds its n_l = units per block * ceil(pixels per
  unit / (4 RPL)) values in turn, the block joins 4 RPL lanes in order; a
  value therefore passes at most L = n_l + 4 RPL additions (the test then
  adds the slab in float64, exactly).  With e = 10 u A per value:
      |sum  - sum64 | <= sum e + L u sum(|v64| + e)
      |sumsq - sq64 | <= sum (2 |v64| e + e^2) + (L + 1) u sum (|v64| + e)^2
  (the +1 is the rounding of fma(v, v, acc)).
* Autograd: on exact data both forward paths give the same y and the same
  BN totals, and the backward code is shared, so every gradient is
  ``torch.equal`` — tighter than the wgrad / BN tests' rounding bounds.
"""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64
STEM_MAX_BLOCKS = 1024
STEM_LDS_FLOATS = 4096

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops import modules as M_ops
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")


def _gen(*tag):
    seed = 0x57E3
    for t in tag:
        seed = (seed * 1000003 + int(t)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _geom(N, H, W, pad):
    """(bands per image, blocks) of the direct kernel's launch."""
    LW = W + 2 * pad
    P = H + 2 * pad - 2
    BP = min(P, STEM_LDS_FLOATS // LW - 2)
    nbands = -(-P // BP)
    Q = W + 2 * pad - 2
    return BP, nbands, min(STEM_MAX_BLOCKS, N * nbands,
                           -(-N * P * Q // 128))


def _xdev(x64):
    return x64.to(BF).contiguous(memory_format=torch.channels_last).to(DEV)


def _poison(shape, dtype):
    """Leave NaNs in the allocator's cache where the next at::empty of this
    size lands: an unwritten slab slot or output row shows."""
    t = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    del t


# ------------------------------------------------------------------ plan ---

FITS = [(1, 28, 28, Ko, pad) for Ko in (8, 16, 64) for pad in (0, 1)]
# N, C, H, W, Ko, R, S, stride, pad
MISFITS = {
    "C3": (2, 3, 28, 28, 64, 3, 3, 1, 1),
    "5x5": (2, 1, 28, 28, 64, 5, 5, 1, 2),
    "stride2": (2, 1, 28, 28, 64, 3, 3, 2, 1),
    "Ko12": (2, 1, 28, 28, 12, 3, 3, 1, 0),
    "Ko128": (2, 1, 28, 28, 128, 3, 3, 1, 0),
}


def test_plan_direct_where_it_fits():
    for N, H, W, Ko, pad in FITS:
        for stem in (-1, 1):
            assert ext.conv2d_stem_plan(N, 1, H, W, Ko, 3, 3, 1, pad,
                                        stem) == "direct"
        assert ext.conv2d_stem_plan(N, 1, H, W, Ko, 3, 3, 1, pad, 0) == "mfma"


@pytest.mark.parametrize("name", sorted(MISFITS))
def test_plan_mfma_for_misfits_even_when_forced(name):
    for stem in (-1, 0, 1):
        assert ext.conv2d_stem_plan(*MISFITS[name], stem) == "mfma"


def test_plan_rejects_a_bad_stem_argument():
    with pytest.raises(RuntimeError):
        ext.conv2d_stem_plan(1, 1, 28, 28, 64, 3, 3, 1, 0, 2)


# ------------------------------------------------------------ exact data ---

def _exact_operands(N, H, W, Ko):
    g = _gen(1, N, H, W, Ko)
    x = torch.randint(-2, 3, (N, 1, H, W), generator=g).to(F64)
    w = torch.randint(-2, 3, (Ko, 1, 3, 3), generator=g).to(F64) / 2
    b = torch.randint(-3, 4, (Ko,), generator=g).to(F64)
    return x, w, b


# 130 images: at 3x3 and 5x7 two to nineteen blocks run up to 65 units each
# with a ragged last trip; 1100 x (3x3) at pad 1: 78 blocks, the last one
# with fewer units; 2 x (40x200, pad 1): three row bands
# per image, the last one 4 rows of 18
EXACT_SHAPES = [(N, H, W, Ko) for N in (1, 3, 130)
                for H, W in ((3, 3), (5, 7), (28, 28)) for Ko in (8, 16, 64)]
EXACT_SHAPES += [(1100, 3, 3, 16), (2, 40, 200, 64), (2, 40, 200, 8)]


@pytest.mark.parametrize("N,H,W,Ko", EXACT_SHAPES,
                         ids=[f"N{a}-{b}x{c}-K{d}"
                              for a, b, c, d in EXACT_SHAPES])
def test_exact_data_both_paths_agree_bit_for_bit(N, H, W, Ko):
    x, w, b = _exact_operands(N, H, W, Ko)
    xd, wd, bd = _xdev(x), w.float().to(DEV), b.float().to(DEV)
    for pad in (0, 1):
        P, Q = H + 2 * pad - 2, W + 2 * pad - 2
        _, nbands, blocks = _geom(N, H, W, pad)
        for bias in (None, bd):
            v = TF.conv2d(x, w, None if bias is None else b, 1, pad)
            assert v.abs().max().item() <= 21
            tot = torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))])
            assert tot.abs().max().item() < 2 ** 22
            for stats in (False, True):
                assert ext.conv2d_stem_plan(N, 1, H, W, Ko, 3, 3, 1, pad,
                                            1) == "direct"
                _poison((2, Ko, blocks), torch.float32)
                _poison((N, P, Q, Ko), BF)
                y1, s1 = ext.conv2d_stem_fwd(xd, wd, bias, 1, pad, stats, 1)
                y0, s0 = ext.conv2d_stem_fwd(xd, wd, bias, 1, pad, stats, 0)
                what = f"pad{pad} bias{bias is not None} stats{stats}"
                assert y1.shape == (N, Ko, P, Q) and y1.dtype == BF
                assert y1.is_contiguous(memory_format=torch.channels_last)
                assert torch.equal(y1, y0), what
                assert torch.equal(y1.cpu().double(), v), what
                if not stats:
                    continue
                # every block has at least one unit: the grid is
                # min(1024, units, 128-pixel tiles), so no slot is left to
                # a block without rows — and none may be left unwritten
                assert s1.shape == (2, Ko, blocks) and blocks <= N * nbands
                assert s0.shape == (2, Ko, -(-N * P * Q // 128))
                t1 = s1.cpu().double().sum(2)
                t0 = s0.cpu().double().sum(2)
                assert torch.equal(t1, t0), what
                assert torch.equal(t1, tot), what


# ----------------------------------------------------------- random data ---

RANDOM_SHAPES = [(3, 5, 7, 8), (130, 28, 28, 64), (1100, 3, 3, 16),
                 (2, 40, 200, 16)]


@pytest.mark.parametrize("N,H,W,Ko", RANDOM_SHAPES,
                         ids=[f"N{a}-{b}x{c}-K{d}"
                              for a, b, c, d in RANDOM_SHAPES])
def test_random_data_within_the_rounding_bounds(N, H, W, Ko):
    g = _gen(2, N, H, W, Ko)
    x = torch.randn(N, 1, H, W, generator=g, dtype=F64).to(BF).double()
    w32 = (torch.randn(Ko, 1, 3, 3, generator=g, dtype=F64) / 3).float()
    w = w32.to(BF).double()
    b = torch.randn(Ko, generator=g, dtype=F64).float().double()
    xd, wd, bd = _xdev(x), w32.to(DEV), b.float().to(DEV)
    rpl = 64 // (Ko // 8)
    for pad in (0, 1):
        BP, nbands, blocks = _geom(N, H, W, pad)
        Q = W + 2 * pad - 2
        v = TF.conv2d(x, w, b, 1, pad)
        A = TF.conv2d(x.abs(), w.abs(), b.abs(), 1, pad)
        y, slab = ext.conv2d_stem_fwd(xd, wd, bd, 1, pad, True, 1)
        yv = y.cpu().double()
        e = 10 * U * A
        hulp = 2.0 ** (torch.floor(torch.log2(v.abs() + e)) - 8)
        bound = hulp + e
        err = (yv - v).abs()
        y0 = ext.conv2d_stem_fwd(xd, wd, bd, 1, pad, False, 0)[0]
        lit = 2.0 ** -9 * v.abs() + e
        print(f"pad{pad}: max err/bound = {(err / bound).max().item():.3f}; "
              f"against 2^-9|v| + e: direct {(err / lit).max().item():.3f}, "
              f"mfma {((y0.cpu().double() - v).abs() / lit).max().item():.3f}")
        assert (err <= bound).all()
        units_per_block = -(-N * nbands // blocks)
        L = units_per_block * -(-BP * Q // (4 * rpl)) + 4 * rpl
        mag = v.abs() + e
        tot = slab.cpu().double().sum(2)
        b_sum = e.sum((0, 2, 3)) + L * U * mag.sum((0, 2, 3))
        b_sq = ((2 * v.abs() * e + e * e).sum((0, 2, 3))
                + (L + 1) * U * (mag * mag).sum((0, 2, 3)))
        e_sum = (tot[0] - v.sum((0, 2, 3))).abs()
        e_sq = (tot[1] - (v * v).sum((0, 2, 3))).abs()
        print(f"pad{pad}: stats err/bound = "
              f"{(e_sum / b_sum).max().item():.3f} "
              f"{(e_sq / b_sq).max().item():.3f}")
        assert (e_sum <= b_sum).all() and (e_sq <= b_sq).all()


# -------------------------------------------------------------- autograd ---

def _conv_bn_step(stem, x, w, b, dy, monkeypatch):
    monkeypatch.setattr(F_ops, "STEM", stem)
    conv = M_ops.Conv2d(1, 16, 3).to(DEV)
    bn = M_ops.BatchNorm2d(16, fuse_relu=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    F_ops.clear_weight_cache()
    out = F_ops.conv_bn(conv, bn, x)
    out.backward(dy)
    return [out.detach(), conv.weight.grad, conv.bias.grad, bn.weight.grad,
            bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone()]


def test_conv_bn_forward_backward_agree_with_the_mfma_path(monkeypatch):
    monkeypatch.delenv("DDPX_STEM", raising=False)
    x64, w64, b64 = _exact_operands(4, 28, 28, 16)
    x = _xdev(x64)
    g = _gen(3)
    dy = _xdev(torch.randint(-2, 3, (4, 16, 26, 26), generator=g).to(F64))
    assert ext.conv2d_stem_plan(4, 1, 28, 28, 16, 3, 3, 1, 0) == "direct"
    got = _conv_bn_step(-1, x, w64.float().to(DEV), b64.float().to(DEV), dy,
                        monkeypatch)
    ref = _conv_bn_step(0, x, w64.float().to(DEV), b64.float().to(DEV), dy,
                        monkeypatch)
    for a, r, name in zip(got, ref, ("out", "dw", "db", "dgamma", "dbeta",
                                     "running_mean", "running_var")):
        assert a is not None and torch.equal(a, r), name
    assert got[1].abs().max().item() > 0


def test_direct_path_reads_the_master_weight_not_a_cached_image():
    x64, w64, b64 = _exact_operands(4, 28, 28, 16)
    x = _xdev(x64)
    conv = M_ops.Conv2d(1, 16, 3).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w64.float().to(DEV))
        conv.bias.copy_(b64.float().to(DEV))
    F_ops.clear_weight_cache()
    with torch.no_grad():
        y_a = conv(x)
        # a write the version counter does not see, then the documented call
        conv.weight.data.mul_(2.0)
        F_ops.clear_weight_cache()
        y_b = conv(x)
        # and one without it: the direct path holds no image to go stale
        conv.weight.data.mul_(0.5)
        y_c = conv(x)
    v = TF.conv2d(x64, w64, b64)
    assert torch.equal(y_a.cpu().double(), v)
    assert torch.equal(y_b.cpu().double(), TF.conv2d(x64, 2 * w64, b64))
    assert not torch.equal(y_a, y_b)
    assert torch.equal(y_c, y_a)
