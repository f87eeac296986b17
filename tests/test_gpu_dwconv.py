"""Depthwise 3x3 kernels (ops/hip/dwconv.hip) against float64 F.conv2d(groups=C)
and its autograd on the CPU; operands are bf16-rounded first.

Notation: u = 2^-24, chunks = C / 8, slw = min(chunks, 64) (slice width),
cb = 256 // slw (columns per block), (slw, tr, gx, gy) = dwconv2d_plan(...).

* Exact data: x, dy in {-2..2}, w in {-1, -1/2, 0, 1/2, 1}, b in {-3..3}: every
  partial sum is exact in fp32 in any order, |v| <= 21 and |dx| <= 18 with one
  fractional bit are exact in bf16, the dw / db / statistics totals stay far
  below 2^24 (asserted on the reference).  y, dx, dw, db and the float64 slab
  totals must then equal float64 (``torch.equal``).
* Random data, forward and dgrad: nine exact products added by an fmaf chain
  from 0, then the bias: |v - v64| <= e = 10 u A, A = sum|x w| + |b|, and
  y = RNE_bf16(v) adds half a bf16 ulp: |y - v64| <= hulp(|v64| + e) + e,
  hulp(t) = 2^(floor(log2 t) - 8) (the bound of test_gpu_stem_fwd.py).
* Random data, wgrad and db: a term passes
      n_l = ceil(units / gx) * tr      fmaf steps of its lane's walk,
                                       units = N ceil(P/tr) ceil(Q/cb),
      cpp + parts                      additions of the block join, parts =
                                       min(cb, max(1, 256 // (8 slw))),
                                       cpp = ceil(cb / parts),
      gx                               additions of the combine if gx <= 64,
      32 + ceil(gx / 32)               else (two stages),
  L in all, the products dy x (8 x 8 bits) are exact, so
      |dw - dw64| <= (L + 1) u sum|dy x|,  |db - db64| <= (L + 1) u sum|dy|.
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
    seed = 0xD3C0
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


def _reference(x, w, b, dy, stride, pad):
    """float64 v, dx, dw, db."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    v = TF.conv2d(x, w, b, stride, pad, groups=x.shape[1])
    v.backward(dy)
    return v.detach(), x.grad, w.grad, b.grad


def _run_kernels(x, w, b, dy, stride, pad, tr=-1):
    """(y, slab, y without bias / stats, dx, dw, db, dw without db), every
    output allocation NaN-poisoned first."""
    N, C, H, W = x.shape
    P, Q = dy.shape[2:]
    xd, dyd = _dev(x), _dev(dy)
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    gx = ext.dwconv2d_plan("fwd", N, C, H, W, stride, pad, tr)[2]
    gw = ext.dwconv2d_plan("wgrad", N, C, H, W, stride, pad, tr)[2]
    _poison(N * C * P * Q, BF)
    _poison(2 * C * gx, torch.float32)
    y, slab = ext.dwconv2d_fwd(xd, wd, bd, stride, pad, True, tr)
    assert slab.shape == (2, C, gx)
    _poison(N * C * P * Q, BF)
    y0, none = ext.dwconv2d_fwd(xd, wd, None, stride, pad, False, tr)
    assert none is None
    _poison(N * C * H * W, BF)
    dx = ext.dwconv2d_dgrad(dyd, wd, H, W, stride, pad, tr)
    for t, hw in ((y, (P, Q)), (y0, (P, Q)), (dx, (H, W))):
        assert t.shape == (N, C) + hw and t.dtype == BF
        assert t.is_contiguous(memory_format=CL)
    _poison(gw * 10 * C, torch.float32)
    _poison(C * 9, torch.float32)
    dw, db = ext.dwconv2d_wgrad(dyd, xd, stride, pad, True, tr)
    _poison(gw * 9 * C, torch.float32)
    dw0, none = ext.dwconv2d_wgrad(dyd, xd, stride, pad, False, tr)
    assert none is None and dw.shape == dw0.shape == (C, 1, 3, 3)
    return [t.cpu().double() for t in (y, slab, y0, dx, dw, db, dw0)]


# ------------------------------------------------------------ exact data ---

# C: one chunk; a chunk count that does not divide 64; two channel slices
# (65 chunks = 64 + 1).  (N, H, W, tr): P = Q = 1 at pad 0; odd extents; a last
# row and column that stride 2 at pad 0 leaves unread; strip tail (P = 37 ->
# 3 x 13, P = 19 -> 2 x 10) with a wave tail (Q * chunks = 135, 129, 69, 66 at
# C = 24) and, at C = 520 (cb = 4), a ragged last column tile; tr = 1 with
# 16 * 24 * 6 = 2304 units (stride 1) so blocks of the 1536-wide grid take a
# second unit.
SMALL = [(1, 3, 3, -1), (3, 5, 7, -1), (2, 8, 8, -1)]
CASES = [(s, p, C) + shp for s in (1, 2) for p in (0, 1) for C in (8, 24, 520)
         for shp in SMALL]
CASES += [(s, p, C, 2, 37, 45, -1) for s in (1, 2) for p in (0, 1)
          for C in (24, 520)]
CASES += [(s, 1, 520, 16, 24, 24, 1) for s in (1, 2)]


@pytest.mark.parametrize("stride,pad,C,N,H,W,tr", CASES,
                         ids=["s{}p{}-C{}-N{}-{}x{}-tr{}".format(*c)
                              for c in CASES])
def test_exact_data_equals_float64(stride, pad, C, N, H, W, tr):
    g = _gen(1, stride, pad, C, N, H, W)
    P, Q = _out_hw(H, W, stride, pad)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).to(F64) / 2
    b = torch.randint(-3, 4, (C,), generator=g).to(F64)
    dy = torch.randint(-2, 3, (N, C, P, Q), generator=g).to(F64)
    v, dx64, dw64, db64 = _reference(x, w, b, dy, stride, pad)
    tot = torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))])
    assert v.abs().max() <= 21 and dx64.abs().max() <= 18
    assert max(tot.abs().max(), dw64.abs().max(), db64.abs().max()) < 2 ** 22
    y, slab, y0, dx, dw, db, dw0 = _run_kernels(x, w, b, dy, stride, pad, tr)
    assert torch.equal(y, v)
    assert torch.equal(y0, v - b.view(1, C, 1, 1))
    assert torch.equal(slab.sum(2), tot)
    assert torch.equal(dx, dx64)
    assert torch.equal(dw, dw64) and torch.equal(dw0, dw64)
    assert torch.equal(db, db64)


# ----------------------------------------------------------- random data ---

def _wgrad_chain(N, C, H, W, stride, pad):
    slw, tr, gx, _ = ext.dwconv2d_plan("wgrad", N, C, H, W, stride, pad)
    P, Q = _out_hw(H, W, stride, pad)
    cb = 256 // slw
    units = N * -(-P // tr) * -(-Q // cb)
    parts = min(cb, max(1, 256 // (8 * slw)))
    join = -(-cb // parts) + parts
    combine = gx if gx <= 64 else 32 + -(-gx // 32)
    return -(-units // gx) * tr + join + combine


@pytest.mark.parametrize("stride,pad,C,N,H,W",
                         [(1, 1, 24, 2, 37, 45), (2, 1, 520, 2, 37, 45)])
def test_random_data_within_the_rounding_bounds(stride, pad, C, N, H, W):
    g = _gen(2, stride, pad, C, N, H, W)
    P, Q = _out_hw(H, W, stride, pad)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64).to(BF).double()
    w32 = (torch.randn(C, 1, 3, 3, generator=g, dtype=F64) / 3).float()
    w = w32.to(BF).double()
    b = torch.randn(C, generator=g, dtype=F64).float().double()
    dy = torch.randn(N, C, P, Q, generator=g, dtype=F64).to(BF).double()
    v, dx64, dw64, db64 = _reference(x, w, b, dy, stride, pad)
    _, dxa, dwa, dba = _reference(x.abs(), w.abs(), b.abs(), dy.abs(), stride,
                                  pad)
    A = TF.conv2d(x.abs(), w.abs(), b.abs(), stride, pad, groups=C)
    y, _, _, dx, dw, db, dw0 = _run_kernels(x, w32.double(), b, dy, stride,
                                            pad)

    def rounded(got, ref, mag):
        e = 10 * U * mag
        bound = 2.0 ** (torch.floor(torch.log2(ref.abs() + e)) - 8) + e
        return ((got - ref).abs() / bound).max().item()
    L = _wgrad_chain(N, C, H, W, stride, pad)
    ratios = {"y": rounded(y, v, A), "dx": rounded(dx, dx64, dxa),
              "dw": ((dw - dw64).abs() / ((L + 1) * U * dwa)).max().item(),
              "db": ((db - db64).abs() / ((L + 1) * U * dba)).max().item()}
    print(f"L = {L}; worst error / bound: {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert torch.equal(dw0, dw)


# ------------------------------------------------------ public interface ---

def _exact_module(C, stride, pad, g):
    conv = M_ops.Conv2d(C, C, 3, stride, pad, groups=C)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, (C, 1, 3, 3), generator=g) / 2)
        conv.bias.copy_(torch.randint(-3, 4, (C,), generator=g))
    return conv


@pytest.mark.parametrize("stride,pad", [(1, 1), (2, 0)])
def test_module_forward_backward_equals_the_float64_module(stride, pad):
    C, N, H, W = 24, 3, 8, 9
    g = _gen(3, stride, pad)
    conv = _exact_module(C, stride, pad, g)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (N, C) + _out_hw(H, W, stride, pad),
                       generator=g).float()
    ref = torch.nn.Conv2d(C, C, 3, stride, pad, groups=C).double()
    ref.load_state_dict(conv.state_dict())
    x64 = x.double().requires_grad_(True)
    ref(x64).backward(dy.double())
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd)
    out.backward(dy.to(DEV))
    assert xd.grad.dtype == torch.float32
    assert torch.equal(out.detach().cpu().double(), ref(x64).detach())
    for got, want in ((xd.grad, x64.grad), (conv.weight.grad, ref.weight.grad),
                      (conv.bias.grad, ref.bias.grad)):
        assert torch.equal(got.cpu().double(), want)


def test_conv_bn_equals_bn_of_conv():
    C, N, H, W = 24, 4, 9, 10
    g = _gen(4)
    conv = _exact_module(C, 1, 1, g).to(DEV)
    x = _dev(torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64))
    dy = _dev(torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64))
    res = []
    for fused in (True, False):
        bn = M_ops.BatchNorm2d(C, fuse_relu=True).to(DEV).train()
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


@pytest.mark.parametrize("kw", [dict(groups=2), dict(dilation=2)])
def test_unsupported_grouped_or_dilated_conv_raises(kw):
    conv = M_ops.Conv2d(16, 16, 3, padding=1, **kw).to(DEV)
    with pytest.raises(ValueError, match="depthwise"):
        conv(torch.zeros(1, 16, 8, 8, device=DEV))


@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
def test_plan_is_a_function_of_the_shape(op):
    shape = (4, 520, 37, 45, 2, 1)
    slw, tr, gx, gy = plan = ext.dwconv2d_plan(op, *shape)
    assert plan == ext.dwconv2d_plan(op, *shape)
    assert (slw, gy) == (64, 2) and 1 <= tr <= 16 and 1 <= gx
    x = torch.zeros(shape[:4], dtype=BF, device=DEV).contiguous(
        memory_format=CL)
    w = torch.zeros(520, 1, 3, 3, device=DEV)
    assert ext.dwconv2d_fwd(x, w, None, 2, 1, True)[1].shape[2] == \
        ext.dwconv2d_plan("fwd", *shape)[2]


# ------------------------------------------------------------- MobileNetV1 ---

def test_mobilenet_training_step_is_bitwise_repeatable():
    x = torch.randn(4, 3, 32, 32, generator=_gen(5)).to(DEV)
    t = torch.tensor([1, 3, 5, 7], device=DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build_model("mobilenet_v1", num_classes=10, cifar_stem=True,
                            width_mult=0.25).to(DEV).train()
        F_ops.clear_weight_cache()
        loss = F_ops.cross_entropy_loss(model(x), t)
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in model.parameters()])
    assert bool(runs[0][0].isfinite()) and len(runs[0]) == 1 + 83
    assert all(g is not None and bool(g.isfinite().all()) for g in runs[0])
    assert runs[0][4].abs().max() > 0          # blocks.0.dw.weight
    for a, r in zip(*runs):
        assert torch.equal(a, r)
