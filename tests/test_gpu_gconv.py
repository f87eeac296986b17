"""Grouped 3x3 MFMA kernels (ops/hip/gconv.hip) against float64
F.conv2d(groups=) and its autograd on the CPU; operands are bf16-rounded first.

Notation: u = 2^-24, Cg = C / groups, (name, row tile, gx, gy, gz, split) =
gconv2d_plan(...).

* Exact data: x, dy in {-2..2}, w in {-1, -1/2, 0, 1/2, 1}, b in {-3..3}.
  Every product is a multiple of 1/2 (1/4 for the squares of the statistics);
  asserted on the reference alone: sum|x w| + |b| (the largest partial sum of
  any order) < 2^24 halves, the per-channel sum|v| and sum v^2 < 2^24 halves /
  quarters, sum|dy x| < 2^24.  Then every fp32 partial sum is exact in any
  order and y, dx must equal the float64 value rounded once to bf16, dw and
  the slab's column totals float64 itself.  These hold for Cg = 64 without
  shrinking the value sets (9 * 64 * 2 + 3 = 1155).
* Random data, forward and dgrad: exact bf16 products and a chain of at most
  9 Cg + 1 fp32 additions: |v - v64| <= e = (9 Cg + 2) u A, A = sum|x w| + |b|
  (sum|dy w| for dx), and the bf16 rounding adds half an ulp:
  |y - v64| <= hulp(|v64| + e) + e, hulp(t) = 2^(floor(log2 t) - 8).
* Random data, wgrad: block (span, split) takes the 64-row tiles split,
  split + S, ...: ceil(tiles / S) tiles, each adding 64 products to the
  accumulator (two 32-deep MFMAs; their inner order is not relied on, every
  product counts as one addition), then the combine adds S partials in one
  chain if S <= 64, else 32 and ceil(S / 32):
      L = 64 ceil(tiles / S) + (S if S <= 64 else 32 + ceil(S / 32)),
      |dw - dw64| <= (L + 1) u sum|dy x|.
"""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64
CL = torch.channels_last

if torch.cuda.is_available():
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops import modules as M_ops
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")


def _gen(*tag):
    seed = 0x6C0F
    for t in tag:
        seed = (seed * 1000003 + int(t)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _dev(t64):
    return t64.to(BF).contiguous(memory_format=CL).to(DEV)


def _poison(numel, dtype):
    """NaNs in the allocator's cache where the next at::empty of this size
    lands: an unwritten output element or slab slot shows."""
    t = torch.full((numel,), float("nan"), dtype=dtype, device=DEV)
    del t


def _out_hw(H, W, stride, pad):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


def _reference(x, w, b, dy, stride, pad, groups):
    """float64 v, dx, dw."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    v = TF.conv2d(x, w, b, stride, pad, groups=groups)
    v.backward(dy)
    return v.detach(), x.grad, w.grad


def _run_kernels(x, w, b, dy, stride, pad, groups):
    """(y with bias and stats, slab, y with bias, y without bias, dx, dw),
    every output allocation NaN-poisoned first."""
    N, C, H, W = x.shape
    P, Q = dy.shape[2:]
    xd, dyd = _dev(x), _dev(dy)
    bd = b.float().to(DEV)
    shape = (N, C, H, W, groups, stride, pad)
    tiles = ext.gconv2d_plan("fwd", *shape)[2]
    split = ext.gconv2d_plan("wgrad", *shape)[5]
    img, img_t = ext.gconv2d_pack(w.float().to(DEV))
    fwd = []
    for bias, stats in ((bd, True), (bd, False), (None, True)):
        _poison(N * C * P * Q, BF)
        _poison(2 * C * tiles, torch.float32)
        fwd.append(ext.gconv2d_fwd(xd, img, bias, groups, stride, pad, stats))
    (y, slab), (y1, none), (y0, _) = fwd
    assert none is None and slab.shape == (2, C, tiles)
    _poison(N * C * H * W, BF)
    dx = ext.gconv2d_dgrad(dyd, img_t, H, W, groups, stride, pad)
    for t, hw in ((y, (P, Q)), (y1, (P, Q)), (y0, (P, Q)), (dx, (H, W))):
        assert t.shape == (N, C) + hw and t.dtype == BF
        assert t.is_contiguous(memory_format=CL)
    _poison(split * C * (C // groups) * 9, torch.float32)
    _poison(C * (C // groups) * 9, torch.float32)
    dw = ext.gconv2d_wgrad(dyd, xd, groups, stride, pad)
    assert dw.shape == w.shape
    return [t.cpu().double() for t in (y, slab, y1, y0, dx, dw)]


# ------------------------------------------------------------ exact data ---

# (C, N, H, W): N P Q = 1 at pad 0; odd extents, one ragged row tile; even
# extents (stride 2 at pad 0 leaves the last dx row and column unread, at
# pad 1 the classes differ in size); three spans with two full row tiles and
# a ragged third at stride 1.  Cg = 64 at C = 64 is a dense conv (groups = 1),
# so there one span becomes two.  Last: the wgrad split is deep enough for the
# two-stage combine, with a ragged last tile and blocks of unequal tile
# counts (asserted from the plan), 135 forward row tiles.
SHAPES = [(64, 1, 3, 3), (64, 3, 5, 7), (64, 2, 8, 10), (192, 2, 13, 11)]
CASES = [(cg, s, p, max(shp[0], 2 * cg)) + shp[1:]
         for cg in (4, 8, 16, 32, 64) for s in (1, 2) for p in (0, 1)
         for shp in SHAPES]
DEEP = (4, 1, 1, 64, 5, 47, 73)
CASES.append(DEEP)


@pytest.mark.parametrize("Cg,stride,pad,C,N,H,W", CASES,
                         ids=["Cg{}-s{}p{}-C{}-N{}-{}x{}".format(*c)
                              for c in CASES])
def test_exact_data_equals_float64(Cg, stride, pad, C, N, H, W):
    g = _gen(1, Cg, stride, pad, C, N, H, W)
    groups = C // Cg
    P, Q = _out_hw(H, W, stride, pad)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    w = torch.randint(-2, 3, (C, Cg, 3, 3), generator=g).to(F64) / 2
    b = torch.randint(-3, 4, (C,), generator=g).to(F64)
    dy = torch.randint(-2, 3, (N, C, P, Q), generator=g).to(F64)
    v, dx64, dw64 = _reference(x, w, b, dy, stride, pad, groups)
    tot = torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))])
    assert 2 * (9 * Cg * 2 + 3) < 2 ** 24 and 4 * N * P * Q < 2 ** 24
    assert 2 * v.abs().sum((0, 2, 3)).max() < 2 ** 24
    assert 4 * tot[1].max() < 2 ** 24
    if (Cg, stride, pad, C, N, H, W) == DEEP:
        _, tile, _, _, _, split = ext.gconv2d_plan("wgrad", N, C, H, W,
                                                    groups, stride, pad)
        tiles = -(-N * P * Q // tile)
        assert split > 64 and tiles % split and (N * P * Q) % tile
    y, slab, y1, y0, dx, dw = _run_kernels(x, w, b, dy, stride, pad, groups)
    assert torch.equal(y, v.to(BF).double())
    assert torch.equal(y1, y)
    assert torch.equal(y0, (v - b.view(1, C, 1, 1)).to(BF).double())
    assert torch.equal(slab.sum(2), tot)
    assert torch.equal(dx, dx64.to(BF).double())
    assert torch.equal(dw, dw64)


# ----------------------------------------------------------- random data ---

def _wgrad_chain(N, C, H, W, groups, stride, pad):
    _, tile, _, _, _, S = ext.gconv2d_plan("wgrad", N, C, H, W, groups,
                                           stride, pad)
    P, Q = _out_hw(H, W, stride, pad)
    tiles = -(-N * P * Q // tile)
    return tile * -(-tiles // S) + (S if S <= 64 else 32 + -(-S // 32))


@pytest.mark.parametrize("Cg,stride,pad,C,N,H,W",
                         [DEEP, (32, 2, 1, 192, 2, 13, 11),
                          (64, 1, 0, 128, 3, 9, 10)])
def test_random_data_within_the_rounding_bounds(Cg, stride, pad, C, N, H, W):
    g = _gen(2, Cg, stride, pad, C, N, H, W)
    groups = C // Cg
    P, Q = _out_hw(H, W, stride, pad)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64).to(BF).double()
    w32 = (torch.randn(C, Cg, 3, 3, generator=g, dtype=F64) / 3).float()
    w = w32.to(BF).double()
    b = torch.randn(C, generator=g, dtype=F64).float().double()
    dy = torch.randn(N, C, P, Q, generator=g, dtype=F64).to(BF).double()
    v, dx64, dw64 = _reference(x, w, b, dy, stride, pad, groups)
    A, dxa, dwa = _reference(x.abs(), w.abs(), b.abs(), dy.abs(), stride, pad,
                             groups)
    y, _, _, _, dx, dw = _run_kernels(x, w32.double(), b, dy, stride, pad,
                                      groups)

    def rounded(got, ref, mag):
        e = (9 * Cg + 2) * U * mag
        bound = 2.0 ** (torch.floor(torch.log2(ref.abs() + e)) - 8) + e
        return ((got - ref).abs() / bound).max().item()
    L = _wgrad_chain(N, C, H, W, groups, stride, pad)
    ratios = {"y": rounded(y, v, A), "dx": rounded(dx, dx64, dxa),
              "dw": ((dw - dw64).abs() / ((L + 1) * U * dwa)).max().item()}
    print(f"L = {L}; worst error / bound: {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios


# ------------------------------------------------------ public interface ---

def _exact_module(C, stride, groups, g):
    conv = M_ops.Conv2d(C, C, 3, stride, 1, groups=groups)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, conv.weight.shape,
                                        generator=g) / 2)
        conv.bias.copy_(torch.randint(-3, 4, (C,), generator=g))
    return conv


@pytest.mark.parametrize("stride,C,groups", [(1, 64, 16), (2, 128, 4)])
def test_module_forward_backward_equals_the_float64_module(stride, C, groups):
    N, H, W = 3, 8, 9
    g = _gen(3, stride, C, groups)
    conv = _exact_module(C, stride, groups, g)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (N, C) + _out_hw(H, W, stride, 1),
                       generator=g).float()
    ref = torch.nn.Conv2d(C, C, 3, stride, 1, groups=groups).double()
    ref.load_state_dict(conv.state_dict())
    x64 = x.double().requires_grad_(True)
    out64 = ref(x64)
    out64.backward(dy.double())
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd)
    out.backward(dy.to(DEV))
    assert xd.grad.dtype == torch.float32
    assert torch.equal(out.detach().cpu().double(),
                       out64.detach().to(BF).double())
    assert torch.equal(xd.grad.cpu().double(), x64.grad.to(BF).double())
    assert torch.equal(conv.weight.grad.cpu().double(), ref.weight.grad)
    assert torch.equal(conv.bias.grad.cpu().double(), ref.bias.grad)


def test_conv_bn_equals_bn_of_conv_and_hands_the_bn_a_slab():
    C, groups, N, H, W = 128, 16, 4, 9, 10
    g = _gen(4)
    conv = _exact_module(C, 1, groups, g).to(DEV)
    x = _dev(torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64))
    dy = _dev(torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64))
    res, seen = [], []
    for fused in (True, False):
        bn = M_ops.BatchNorm2d(C, fuse_relu=True).to(DEV).train()
        inner = bn.forward
        bn.forward = lambda y, _f=inner, **kw: (
            seen.append(kw.get("pre_stats")), _f(y, **kw))[1]
        conv.zero_grad()
        xr = x.clone().requires_grad_(True)
        out = F_ops.conv_bn(conv, bn, xr) if fused else bn(conv(xr))
        out.backward(dy)
        res.append([out.detach(), xr.grad, conv.weight.grad.clone(),
                    conv.bias.grad.clone(), bn.weight.grad, bn.bias.grad,
                    bn.running_mean, bn.running_var])
    for a, r in zip(*res):
        assert torch.equal(a, r)
    assert res[0][2].abs().max() > 0 and bool(res[0][0].isfinite().all())
    tiles = ext.gconv2d_plan("fwd", N, C, H, W, groups, 1, 1)[2]
    assert seen[0].shape == (2, C, tiles) and seen[1] is None


@pytest.mark.parametrize("cin,cout,k,kw", [
    (96, 96, 3, dict(groups=12)),              # C % 64 != 0
    (64, 128, 3, dict(groups=8)),              # C_in != C_out
    (64, 64, 5, dict(groups=8)),               # 5x5
    (64, 64, 3, dict(groups=32)),              # Cg = 2
    (64, 64, 3, dict(groups=8, dilation=2)),
])
def test_out_of_scope_grouped_conv_raises(cin, cout, k, kw):
    conv = M_ops.Conv2d(cin, cout, k, padding=1, **kw).to(DEV)
    with pytest.raises(ValueError, match="depthwise.*grouped"):
        conv(torch.zeros(1, cin, 8, 8, device=DEV))


def test_resnext_training_step_is_bitwise_repeatable():
    x = torch.randn(8, 3, 32, 32, generator=_gen(5)).to(DEV)
    t = torch.arange(8, device=DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build_model("resnext50_32x4d", num_classes=10,
                            cifar_stem=True).to(DEV).train()
        F_ops.clear_weight_cache()
        loss = F_ops.cross_entropy_loss(model(x), t)
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in model.parameters()])
    assert bool(runs[0][0].isfinite()) and len(runs[0]) == 1 + 161
    assert all(g is not None and bool(g.isfinite().all()) and
               g.abs().max() > 0 for g in runs[0])
    for a, r in zip(*runs):
        assert torch.equal(a, r)
