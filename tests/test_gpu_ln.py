"""LayerNorm, GELU and layer-scale kernels (ops/hip/ln.hip) against float64
formulas on the CPU over the bf16-rounded operands.

Notation: u = 2^-24, hulp(t) = 2^(floor(log2 t) - 8), (lpr, cpl, rpg, grid) =
ln2d_plan(M, C, blocks), M = N H W, L = 8 cpl + log2(lpr) the additions a term
of a row sum passes (the lane's chain, then the tree).  A bf16 output y of a
value v64 computed with first-order error e must satisfy
|y - v64| <= hulp(|v64| + e) + e; e carries the factor 1.01 for the dropped
second-order terms.  fp32 outputs must lie within 1.01 e.

LayerNorm forward, in the kernel's order (sum, mean = sum / C, d = x - mean,
sum of fma(d, d, .), var = . / C, rstd = 1 / sqrt(var + eps),
y = fma(d rstd, gamma, beta)):
    dmu  = L u sum|x| / C + u |mean64|
    dvar = (L + 3) u var64 + 2 dmu sum|x - mean64| / C
    dis  = dvar / 2 (var64 + eps)^(-3/2) + 4 u rstd64
    e_y  = |gamma| (|x - mean64| dis + (rstd64 + dis) dmu)
           + 3 u |gamma xhat64| + u |v64|
and the saved mean / rstd lie within dmu / dis.

LayerNorm backward (xhat = (x - mean) rstd, g = dy gamma, s1 = sum g,
s2 = sum fma(g, xhat, .), a1 = s1 / C, a2 = s2 / C, t = fma(xhat, a2, a1),
w = g - t, dx = rstd w):
    dxh  = |x - mean64| dis + rstd64 dmu + 2 u |xhat64|
    ds1  = (L + 1) u sum|g|
    ds2  = (L + 1) u sum|g xhat| + sum |g| dxh
    dt   = (ds1 + u |s1| + |xhat| (ds2 + u |s2|) + dxh |s2|) / C + u |t|
    e_dx = dis |w| + rstd64 (u |g| + dt + u |w|) + u |dx64|
A term of dbeta / dgamma passes ceil(groups / grid) additions in its lane,
rpg in the block join and one rounding after the double combine, K in all:
    e_dbeta  = K u sum|dy|
    e_dgamma = (K + 1) u sum|dy xhat| + sum |dy| dxh

Exact data: every row of x holds m0 + a and m0 - a in equal numbers (integers,
|x| <= 6), dy is integer in {-2..2}: the row sum is exact, so the saved mean
is m0, and the dbeta sums are exact at every block count.

GELU: e = 8 u |z| forward, 8 u |dy| (1 + |z|) backward (erf and exp within
4 ulp; the kernel's ln_erf, emulated in fp32 over every bf16 input, errs by
at most 1.2 u).  Layer scale: e = 2 u (|gamma u| + |resid|), 2 u |gamma dy| for du,
dgamma as dbeta above with the exact products dy u, exact on integer data.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-6
BF = torch.bfloat16
F64 = torch.float64
CL = torch.channels_last

if torch.cuda.is_available():
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops import modules as M_ops
    from ddp_tricks_amd.ops.optim import FusedAdamW
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")


def _gen(*tag):
    seed = 0x1A7E
    for t in tag:
        seed = (seed * 1000003 + int(t) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.to(BF).to(F64)


def _dev(t64):
    t = t64.to(BF)
    return (t.contiguous(memory_format=CL) if t.dim() == 4 else t).to(DEV)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu().to(F64)


def _within(got, ref, e):
    e = 1.01 * e
    hulp = torch.exp2(torch.floor(torch.log2((ref.abs() + e).clamp_min(1e-300))) - 8)
    assert bool(((got - ref).abs() <= hulp + e).all())


def _within32(got, ref, e):
    assert bool(((got.cpu().to(F64) - ref).abs() <= 1.01 * e).all())


def _chain(M, C, blocks):
    lpr, cpl, rpg, grid = ext.ln2d_plan(M, C, blocks)
    groups = (M + rpg - 1) // rpg
    return 8 * cpl + math.log2(lpr), (groups + grid - 1) // grid + rpg + 1


def _check_ln(x, gam, bet, dy, blocks):
    """Runs the kernels on float64 operands (already bf16 / fp32 values) and
    holds every output to the docstring's bounds; returns (mean, dbeta)."""
    C = x.shape[1]
    X, DY = _rows(x), _rows(dy)
    M = X.shape[0]
    L, K = _chain(M, C, blocks)
    mu = X.mean(1, keepdim=True)
    d = X - mu
    var = d.square().mean(1, keepdim=True)
    rs = (var + EPS).rsqrt()
    xh = d * rs
    v = xh * gam + bet
    dmu = L * U * X.abs().mean(1, keepdim=True) + U * mu.abs()
    dvar = (L + 3) * U * var + 2 * dmu * d.abs().mean(1, keepdim=True)
    dis = dvar / 2 * (var + EPS) ** -1.5 + 4 * U * rs
    e_y = (gam.abs() * (d.abs() * dis + (rs + dis) * dmu)
           + 3 * U * (gam * xh).abs() + U * v.abs())
    g = DY * gam
    s1 = g.sum(1, keepdim=True)
    s2 = (g * xh).sum(1, keepdim=True)
    t = (s1 + xh * s2) / C
    w = g - t
    dxh = d.abs() * dis + rs * dmu + 2 * U * xh.abs()
    ds1 = (L + 1) * U * g.abs().sum(1, keepdim=True)
    ds2 = ((L + 1) * U * (g * xh).abs().sum(1, keepdim=True)
           + (g.abs() * dxh).sum(1, keepdim=True))
    dt = (ds1 + U * s1.abs() + xh.abs() * (ds2 + U * s2.abs())
          + dxh * s2.abs()) / C + U * t.abs()
    e_dx = dis * w.abs() + rs * (U * g.abs() + dt + U * w.abs()) + U * (rs * w).abs()

    xd, dyd = _dev(x), _dev(dy)
    gd, bd = gam.float().to(DEV), bet.float().to(DEV)
    y, mean, rstd = ext.ln2d_fwd(xd, gd, bd, EPS, True, blocks)
    y0, m0, r0 = ext.ln2d_fwd(xd, gd, bd, EPS, False, blocks)
    assert torch.equal(y0, y) and m0.numel() == r0.numel() == 0
    assert y.dtype == BF and y.is_contiguous(memory_format=CL)
    dx, dg, db = ext.ln2d_bwd(xd, dyd, gd, mean, rstd, blocks)
    _within(_rows(y), v, e_y)
    _within32(mean, mu[:, 0], dmu[:, 0])
    _within32(rstd, rs[:, 0], dis[:, 0])
    _within(_rows(dx), rs * w, e_dx)
    _within32(db, DY.sum(0), K * U * DY.abs().sum(0))
    _within32(dg, (DY * xh).sum(0), (K + 1) * U * (DY * xh).abs().sum(0)
              + (DY.abs() * dxh).sum(0))
    return mean.cpu(), db.cpu()


# (N, C, H, W, blocks): C = 8 lpr 1; 24 lpr 4 with an idle lane; 96 12 of 16
# lanes; 384 48 of 64; 520 cpl 2 with one live chunk in the second slot; 768
# cpl 2; 1280 cpl 4 with a dead slot; 2048 cpl 4 full.  M = 35 is no multiple
# of any rpg; blocks 1 / 3 force the grid-stride walk and the multi-block
# join; the last case puts two blocks on one chain of the combine.
LN_CASES = [(1, 8, 5, 7, -1), (3, 8, 17, 11, 3), (1, 24, 5, 7, 1),
            (2, 24, 9, 11, 1), (2, 96, 5, 7, 3), (1, 384, 5, 7, 3),
            (1, 520, 5, 7, 3), (1, 768, 5, 7, 1), (1, 1280, 3, 3, -1),
            (1, 2048, 5, 7, 3), (2, 96, 20, 20, 20)]


@pytest.mark.parametrize("N,C,H,W,blocks", LN_CASES)
def test_layer_norm_within_rounding_bounds(N, C, H, W, blocks):
    g = _gen(N, C, H, blocks)
    x = _bf(torch.randn(N, C, H, W, generator=g, dtype=F64) + 0.5)
    dy = _bf(torch.randn(N, C, H, W, generator=g, dtype=F64))
    gam = (1 + 0.5 * torch.randn(C, generator=g)).to(F64)
    bet = (0.5 * torch.randn(C, generator=g)).to(F64)
    _check_ln(x, gam, bet, dy, blocks)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("N,C,H,W", [(3, 8, 17, 11), (2, 96, 5, 7),
                                     (1, 520, 5, 7)])
def test_layer_norm_exact_data(N, C, H, W, blocks):
    g = _gen(N, C, blocks, 1)
    M = N * H * W
    m0 = torch.randint(-2, 3, (M, 1), generator=g).to(F64)
    a = torch.tensor([1.0, 2.0, 4.0], dtype=F64)[
        torch.randint(0, 3, (M, 1), generator=g)]
    sign = torch.cat([torch.ones(M, C // 2), -torch.ones(M, C // 2)], 1)
    sign = torch.gather(sign, 1, torch.rand(M, C, generator=g).argsort(1))
    x = (m0 + a * sign.to(F64)).view(N, H, W, C).permute(0, 3, 1, 2)
    dy = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    gam = (1 + 0.5 * torch.randn(C, generator=g)).to(F64)
    bet = (0.5 * torch.randn(C, generator=g)).to(F64)
    mean, db = _check_ln(x, gam, bet, dy, blocks)
    assert torch.equal(mean.to(F64), m0[:, 0])
    assert torch.equal(db.to(F64), _rows(dy).sum(0))


# 8 elements; a block's 256 chunks plus one; past the 2048-block grid
@pytest.mark.parametrize("n", [8, 256 * 8 + 8, 2048 * 256 * 8 + 40])
def test_gelu(n):
    g = _gen(n)
    z = 2 * torch.randn(n, generator=g, dtype=F64)
    pts = torch.tensor([0, 0.5, -0.5, 3, -3, 6, -6, 10, -10], dtype=F64)[:n]
    z[:len(pts)] = pts
    z = _bf(z)
    dy = _bf(torch.randn(n, generator=g, dtype=F64))
    cdf = 0.5 * torch.special.erfc(-z / math.sqrt(2))
    pdf = torch.exp(-z * z / 2) / math.sqrt(2 * math.pi)
    zd = _dev(z)
    a = ext.gelu_fwd(zd)
    dz = ext.gelu_bwd(_dev(dy), zd)
    assert a.dtype == dz.dtype == BF and a.shape == dz.shape == (n,)
    _within(a.cpu().to(F64), z * cdf, 8 * U * z.abs())
    _within(dz.cpu().to(F64), dy * (cdf + z * pdf),
            8 * U * dy.abs() * (1 + z.abs()))


# the last case walks more row groups than the forward's 2048 blocks
@pytest.mark.parametrize("N,C,H,W,blocks", [
    (1, 24, 5, 7, 1), (2, 96, 9, 11, 3), (1, 520, 5, 7, 3),
    (1, 2048, 3, 3, -1), (2049, 8, 16, 16, -1)])
def test_layer_scale(N, C, H, W, blocks):
    g = _gen(N, C, H, 2)
    M = N * H * W
    _, K = _chain(M, C, blocks)
    gam = (0.5 * torch.randn(C, generator=g)).to(F64)
    gd = gam.float().to(DEV)
    for exact in (False, True):
        if exact:
            u, r, dy = (torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
                        for _ in range(3))
        else:
            u, r, dy = (_bf(torch.randn(N, C, H, W, generator=g, dtype=F64))
                        for _ in range(3))
        ud, rd, dyd = _dev(u), _dev(r), _dev(dy)
        y = ext.lscale_fwd(ud, gd, rd)
        du, dg = ext.lscale_bwd(dyd, ud, gd, blocks)
        assert y.is_contiguous(memory_format=CL) and du.dtype == BF
        U_, R_, DY_ = _rows(u), _rows(r), _rows(dy)
        _within(_rows(y), R_ + gam * U_, 2 * U * ((gam * U_).abs() + R_.abs()))
        _within(_rows(du), gam * DY_, 2 * U * (gam * DY_).abs())
        dg64 = (DY_ * U_).sum(0)
        if exact:
            assert torch.equal(dg.cpu().to(F64), dg64)
        else:
            _within32(dg, dg64, K * U * (DY_ * U_).abs().sum(0))


def test_modules_run_the_bindings_through_autograd():
    g = _gen(3)
    N, C, H, W = 2, 96, 5, 7
    x, r, dy = (_dev(torch.randn(N, C, H, W, generator=g, dtype=F64))
                for _ in range(3))
    w, b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)

    ln = M_ops.LayerNorm2d(C).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    y = ln(xr)
    y.backward(dy)
    yb, mean, rstd = ext.ln2d_fwd(x, w, b, 1e-6, True)
    want = (yb,) + tuple(ext.ln2d_bwd(x, dy, w, mean, rstd))
    for a, e in zip((y, xr.grad, ln.weight.grad, ln.bias.grad), want):
        assert torch.equal(a, e)

    xr = x.clone().requires_grad_(True)
    a = M_ops.GELU()(xr)
    a.backward(dy)
    assert torch.equal(a, ext.gelu_fwd(x))
    assert torch.equal(xr.grad, ext.gelu_bwd(dy, x))

    ls = M_ops.LayerScale(C, init=0.5).to(DEV)
    xr, rr = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y = ls(xr, rr)
    dxr, drr, dgam = torch.autograd.grad(y, (xr, rr, ls.gamma), dy)
    du, dg = ext.lscale_bwd(dy, x, ls.gamma.detach())
    assert torch.equal(y, ext.lscale_fwd(x, ls.gamma.detach(), r))
    assert torch.equal(dxr, du) and torch.equal(dgam, dg)
    assert drr.data_ptr() == dy.data_ptr()      # dy itself, not a copy


@pytest.mark.parametrize("shape", [(2, 12, 4, 4), (1, 2056, 2, 2), (4, 96, 8)])
def test_out_of_scope_inputs_raise(shape):
    x = torch.zeros(shape, device=DEV)
    w = torch.ones(shape[1], device=DEV)
    with pytest.raises(ValueError, match=r"C % 8 == 0 and C <= 2048"):
        F_ops.layer_norm2d(x, w, w)
    with pytest.raises(ValueError, match=r"C % 8 == 0 and C <= 2048"):
        F_ops.layer_scale(x, w, x)


def test_convnext_amp_adamw_step_is_bitwise_repeatable():
    x = torch.randn(8, 3, 32, 32, generator=_gen(5)).to(DEV)
    t = torch.arange(8, device=DEV)
    runs = []
    try:
        for _ in range(2):
            amp._state.__init__()
            F_ops.clear_weight_cache()
            same_seeds(0)
            model = build_model("convnext_tiny", num_classes=10,
                                cifar_stem=True).to(DEV).train()
            opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
            model, opt = amp.initialize(model, opt, opt_level="O1")
            opt.zero_grad()
            loss = F_ops.cross_entropy_loss(model(x), t) / 8
            with amp.scale_loss(loss, opt) as scaled:
                scaled.backward()
            gam = model.stages[2][0].scale.gamma.grad
            assert gam.shape == (384,) and gam.abs().max() > 0
            opt.step()
            runs.append([loss.detach()] + [p.detach().clone()
                                           for p in model.parameters()])
    finally:
        amp._state.__init__()
    assert bool(runs[0][0].isfinite())
    for a, r in zip(*runs):
        assert torch.equal(a, r) and bool(a.isfinite().all())
