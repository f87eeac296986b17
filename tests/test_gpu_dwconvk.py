"""Depthwise 5x5 / 7x7 kernels (ops/hip/dwconvk.hip) against float64
F.conv2d(groups=C) and its autograd on the CPU; operands are bf16-rounded first.

Notation: u = 2^-24, (slw, to, gx, gy) = dwconvk2d_plan(...).

* Exact data: x, dy in {-2..2}, w in {-1, -1/2, 0, 1/2, 1}, b in {-3..3}: every
  partial sum is exact in fp32 in any order, |v| <= 101 and |dx| <= 98 with one
  fractional bit are exact in bf16, the dw / db / statistics totals stay below
  2^22 (asserted on the reference).  y, dx, dw, db and the float64 slab totals
  must then equal float64 (``torch.equal``).
* Random data, forward and dgrad: K^2 exact products added by an fmaf chain
  from 0, then the bias: |v - v64| <= e = (K^2 + 1) u A, A = sum|x w| + |b|,
  and y = RNE_bf16(v) adds half a bf16 ulp: |y - v64| <= hulp(|v64| + e) + e,
  hulp(t) = 2^(floor(log2 t) - 8).
* Random data, wgrad and db: for the wgrad plan `to` is the rows per group; a
  term passes
      ceil(N ceil(P / to) / gx) * Q    fmaf steps of its lane's walk,
      to                               additions of the block join,
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
KS = [(5, 1), (5, 2), (7, 1)]

if torch.cuda.is_available():
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops import modules as M_ops
    from ddp_tricks_amd.ops.optim import FusedSGD
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")


def _gen(*tag):
    seed = 0xD3C5
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


def _out_hw(H, W, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def _reference(x, w, b, dy, stride, pad):
    """float64 v, dx, dw, db."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    v = TF.conv2d(x, w, b, stride, pad, groups=x.shape[1])
    v.backward(dy)
    return v.detach(), x.grad, w.grad, b.grad


def _run_kernels(x, w, b, dy, stride, pad, to=-1):
    """(y, slab, y without bias / stats, dx, dw, db, dw without db), every
    output allocation NaN-poisoned first."""
    N, C, H, W = x.shape
    K = w.shape[-1]
    P, Q = dy.shape[2:]
    xd, dyd = _dev(x), _dev(dy)
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    gx = ext.dwconvk2d_plan("fwd", N, C, H, W, K, stride, pad, to)[2]
    gw = ext.dwconvk2d_plan("wgrad", N, C, H, W, K, stride, pad, to)[2]
    _poison(N * C * P * Q, BF)
    _poison(2 * C * gx, torch.float32)
    y, slab = ext.dwconvk2d_fwd(xd, wd, bd, stride, pad, True, to)
    assert slab.shape == (2, C, gx)
    _poison(N * C * P * Q, BF)
    y0, none = ext.dwconvk2d_fwd(xd, wd, None, stride, pad, False, to)
    assert none is None
    _poison(N * C * H * W, BF)
    dx = ext.dwconvk2d_dgrad(dyd, wd, H, W, stride, pad, to)
    for t, hw in ((y, (P, Q)), (y0, (P, Q)), (dx, (H, W))):
        assert t.shape == (N, C) + hw and t.dtype == BF
        assert t.is_contiguous(memory_format=CL)
    _poison(gw * (K * K + 1) * C, torch.float32)
    _poison(C * K * K, torch.float32)
    dw, db = ext.dwconvk2d_wgrad(dyd, xd, K, stride, pad, True, to)
    _poison(gw * K * K * C, torch.float32)
    dw0, none = ext.dwconvk2d_wgrad(dyd, xd, K, stride, pad, False, to)
    assert none is None and dw.shape == dw0.shape == (C, 1, K, K)
    return [t.cpu().double() for t in (y, slab, y0, dx, dw, db, dw0)]


# ------------------------------------------------------------ exact data ---

# C: one chunk; three chunks (cb = 85, 255 lanes); one chunk past the slice
# width of 16 (two slices on gridDim.y, the second with one chunk).
# (N, H, W): 0 stands for K, so P = Q = 1 at pad 0; odd extents; at K5 stride 2
# pad 0 a last row and column that no output reads (dx there is 0); a ragged
# last row run, a ragged last column tile (C = 136: cb = 16, Q = 37 / 17) and
# a wave tail.  to = 1: 12 * 32 * 3 = 1152 forward units at stride 1 and
# 12 * 32 * 3 at stride 2, past the plan's grid, so blocks take a second unit;
# its wgrad plan has 12 * 32 / 4 = 96 blocks: the two-stage combine.
SHAPES = [(1, 0, 0), (3, 9, 11), (2, 10, 10), (2, 21, 37)]
CASES = [(K, s, p, C) + shp + (-1,) for K, s in KS for p in (0, K // 2)
         for C in (8, 24, 136) for shp in SHAPES]
CASES += [(K, s, K // 2, 136, 12, 32 * s, 40 * s + 2 * (s - 1), 1)
          for K, s in KS]


@pytest.mark.parametrize("K,stride,pad,C,N,H,W,to", CASES,
                         ids=["k{}s{}p{}-C{}-N{}-{}x{}-to{}".format(*c)
                              for c in CASES])
def test_exact_data_equals_float64(K, stride, pad, C, N, H, W, to):
    H, W = H or K, W or K
    g = _gen(1, K, stride, pad, C, N, H, W)
    P, Q = _out_hw(H, W, K, stride, pad)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    w = torch.randint(-2, 3, (C, 1, K, K), generator=g).to(F64) / 2
    b = torch.randint(-3, 4, (C,), generator=g).to(F64)
    dy = torch.randint(-2, 3, (N, C, P, Q), generator=g).to(F64)
    v, dx64, dw64, db64 = _reference(x, w, b, dy, stride, pad)
    tot = torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))])
    assert v.abs().max() <= 101 and dx64.abs().max() <= 98
    assert max(tot.abs().max(), dw64.abs().max(), db64.abs().max()) < 2 ** 22
    if to == 1:
        slw, rows, gx, _ = ext.dwconvk2d_plan("fwd", N, C, H, W, K, stride,
                                              pad, 1)
        assert rows == 1 and N * P * -(-Q // (256 // slw)) > gx
        assert ext.dwconvk2d_plan("wgrad", N, C, H, W, K, stride, pad,
                                  1)[2] > 64
    y, slab, y0, dx, dw, db, dw0 = _run_kernels(x, w, b, dy, stride, pad, to)
    assert torch.equal(y, v)
    assert torch.equal(y0, v - b.view(1, C, 1, 1))
    assert torch.equal(slab.sum(2), tot)
    assert torch.equal(dx, dx64)
    if (K, stride, pad) == (5, 2, 0) and H == 10:
        assert not dx64[:, :, -1].any() and not dx64[:, :, :, -1].any()
    assert torch.equal(dw, dw64) and torch.equal(dw0, dw64)
    assert torch.equal(db, db64)


# ----------------------------------------------------------- random data ---

def _wgrad_chain(N, C, H, W, K, stride, pad):
    _, to, gx, _ = ext.dwconvk2d_plan("wgrad", N, C, H, W, K, stride, pad)
    P, Q = _out_hw(H, W, K, stride, pad)
    units = N * -(-P // to)
    combine = gx if gx <= 64 else 32 + -(-gx // 32)
    return -(-units // gx) * Q + to + combine


@pytest.mark.parametrize("K,stride", KS)
def test_random_data_within_the_rounding_bounds(K, stride):
    C, N, H, W, pad = 24, 2, 21, 37, K // 2
    g = _gen(2, K, stride)
    P, Q = _out_hw(H, W, K, stride, pad)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64).to(BF).double()
    w32 = (torch.randn(C, 1, K, K, generator=g, dtype=F64) / K).float()
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
        e = (K * K + 1) * U * mag
        bound = 2.0 ** (torch.floor(torch.log2(ref.abs() + e)) - 8) + e
        return ((got - ref).abs() / bound).max().item()
    L = _wgrad_chain(N, C, H, W, K, stride, pad)
    ratios = {"y": rounded(y, v, A), "dx": rounded(dx, dx64, dxa),
              "dw": ((dw - dw64).abs() / ((L + 1) * U * dwa)).max().item(),
              "db": ((db - db64).abs() / ((L + 1) * U * dba)).max().item()}
    print(f"L = {L}; worst error / bound: {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert torch.equal(dw0, dw)


# ------------------------------------------------------ public interface ---

def _exact_module(C, K, stride, pad, g):
    conv = M_ops.Conv2d(C, C, K, stride, pad, groups=C)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, (C, 1, K, K), generator=g) / 2)
        conv.bias.copy_(torch.randint(-3, 4, (C,), generator=g))
    return conv


@pytest.mark.parametrize("K,stride,pad", [(5, 1, 2), (5, 2, 0), (7, 1, 3)])
def test_module_forward_backward_equals_the_float64_module(K, stride, pad):
    C, N, H, W = 24, 3, 9, 10
    g = _gen(3, K, stride, pad)
    conv = _exact_module(C, K, stride, pad, g)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (N, C) + _out_hw(H, W, K, stride, pad),
                       generator=g).float()
    ref = torch.nn.Conv2d(C, C, K, stride, pad, groups=C).double()
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
    conv = _exact_module(C, 5, 1, 2, g).to(DEV)
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


# the last case: a 4x16 input under a 5x5 window without padding
@pytest.mark.parametrize("K,stride,pad,H", [(7, 2, 3, 16), (9, 1, 4, 16),
                                            (5, 1, 0, 4)])
def test_out_of_scope_depthwise_conv_raises(K, stride, pad, H):
    conv = M_ops.Conv2d(16, 16, K, stride, pad, groups=16).to(DEV)
    with pytest.raises(ValueError, match="depthwise.*grouped"):
        conv(torch.zeros(1, 16, H, 16, device=DEV))


@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
def test_plan_is_a_function_of_the_shape(op):
    shape = (4, 136, 21, 37, 5, 2, 2)
    slw, to, gx, gy = plan = ext.dwconvk2d_plan(op, *shape)
    assert plan == ext.dwconvk2d_plan(op, *shape)
    assert (slw, gy) == (16, 2) and 1 <= to <= 8 and 1 <= gx
    forced = ext.dwconvk2d_plan(op, *shape, 1)
    assert forced == ext.dwconvk2d_plan(op, *shape, 1) and forced[1] == 1
    x = torch.zeros(shape[:4], dtype=BF, device=DEV).contiguous(
        memory_format=CL)
    w = torch.zeros(136, 1, 5, 5, device=DEV)
    assert ext.dwconvk2d_fwd(x, w, None, 2, 2, True)[1].shape[2] == \
        ext.dwconvk2d_plan("fwd", *shape)[2]


# ---------------------------------------------------------------- MnasNet ---

def test_mnasnet_amp_training_step_is_bitwise_repeatable():
    x = torch.randn(8, 3, 32, 32, generator=_gen(5)).to(DEV)
    t = torch.arange(8, device=DEV)
    runs = []
    try:
        for _ in range(2):
            amp._state.__init__()
            F_ops.clear_weight_cache()
            same_seeds(0)
            model = build_model("mnasnet1_0", num_classes=10,
                                cifar_stem=True).to(DEV).train()
            opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9,
                           nesterov=True)
            model, opt = amp.initialize(model, opt, opt_level="O1")
            opt.zero_grad()
            loss = F_ops.cross_entropy_loss(model(x), t) / 8
            with amp.scale_loss(loss, opt) as scaled:
                scaled.backward()
            dw5 = model.stacks[1][0].dw.weight.grad
            assert dw5.shape == (72, 1, 5, 5) and dw5.abs().max() > 0
            runs.append([loss.detach()] + [p.grad.clone()
                                           for p in model.parameters()])
    finally:
        amp._state.__init__()
    assert bool(runs[0][0].isfinite())
    for a, r in zip(*runs):
        assert torch.equal(a, r) and bool(a.isfinite().all())
