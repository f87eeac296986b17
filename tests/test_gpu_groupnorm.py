"""GroupNorm kernels (ops/hip/gn.hip) against float64 on the CPU over the
bf16-rounded operands.

Notation: u = 2^-24, rows = H W, Cg = C / G, m = rows Cg, (slw, walkers, S,
slices) = gn_plan(...), strip = ceil(rows / S), hulp(t) = 2^(floor(log2 t) - 8)
(half a bf16 ulp), isb = invstd + dis.  Every bound below is first order; the
dropped products of two relative errors (each < 2^-10 at these shapes) are
covered by the factor 1.01 on e and e_dx.

* Statistics.  A lane adds ceil(strip / walkers) terms in fp32 (the squares by
  fma, one rounding each), the join adds `walkers` partials, the combine is in
  double and contributes only its final rounding: with
  L = ceil(strip / walkers) + walkers, a = sum|x| / m, q = sum x^2 / m,
      |mean - mean64| <= dmu = L u a + u |mean64|,
      |var - var64|   <= dvar = L u (q + 2 |mean64| a),
      |invstd - invstd64| <= dis
          = dvar / 2 (max(var64 - dvar, 0) + eps)^-3/2 + u invstd64.
* Forward.  scale = fl(gamma invstd), shift = fl(beta - mean scale), one fma,
  one more rounding with a residual, then bf16:
      e = |gamma| (|x - mean| dis + isb dmu)
          + u (|gamma| isb (|x| + |mean|) + |beta|) + 2 u (|v64| + |resid|),
      |y - relu?(v64)| <= hulp(|v64| + e) + e.
  The mask must equal v64 > 0 wherever |v64| > e; at most 0.1 % of the
  elements may be exempt (asserted on the reference alone).
* Backward, with the kernel's own mask in dy_eff.  xhat = fl(fl(x - mean)
  invstd): dxh = isb dmu + |x - mean| dis + 2 u |xhat|; per (n, c)
      errA = L u sum|dy_eff|,  errB = sum|dy_eff| dxh + L u sum|dy_eff xhat|;
  dbeta, dgamma add these over n in double and round once.  ds1, ds2 are the
  |gamma|-weighted group sums of errA, errB; k1, k2, k3 are rounded once from
  double, dx = fma(k1, dy_eff, fma(k2, x, k3)), then bf16:
      e_dx = |gamma dy_eff| dis
           + ((2 invstd dis + dis^2) |s2| |x - mean| + isb^2 ds2 |x - mean|
              + isb^2 (|s2| + ds2) dmu) / m
           + (dis |s1| + isb ds1) / m
           + u (|k1 dy_eff| + |k2 x| + |k3|) + 2 u (|k2 x + k3| + |dx64|),
      |dx - dx64| <= hulp(|dx64| + e_dx) + e_dx,   dresid = dy_eff exactly.
* Exact data: x, dy in {-2..2}, relu off.  sum|x|, sum|dy| < 2^24 (asserted),
  so every fp32 partial sum is exact in any order: mean is the float64 mean
  rounded once to fp32 and dbeta the float64 sum, at any strip count.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64
CL = torch.channels_last
EPS = 1e-5

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops import modules as M_ops
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

# (N, C, G, H, W, strips): Cg = 2, a chunk spans 4 groups, n-indexed
# coefficients; Cg = 1 and a strip tail; Cg = 8, three strips of 25 rows;
# Cg = 6, groups straddle chunks, 255 of 256 lanes; Cg = 24, slw = 6, idle
# lanes; G = 1; a ResNet shape, 4 walkers; a second channel slice with one
# live chunk.
TABLE = [(3, 8, 4, 5, 5, 1), (2, 8, 8, 3, 7, 2), (2, 16, 2, 5, 5, 3),
         (2, 24, 4, 4, 4, 1), (2, 48, 2, 6, 6, 2), (2, 64, 1, 9, 9, -1),
         (2, 512, 32, 7, 7, -1), (1, 2056, 257, 2, 2, 1)]


def _gen(*tag):
    return torch.Generator().manual_seed(hash(tag) % 2 ** 31)


def _dev(t64):
    return t64.to(BF).contiguous(memory_format=CL).to(DEV)


def _poison(*sizes):
    """NaNs in the allocator's cache where the next at::empty of each size
    lands: an unwritten output element or slab slot shows."""
    for numel, dtype in sizes:
        t = torch.full((numel,), float("nan"), dtype=dtype, device=DEV)
        del t


def _hulp(t):
    return 2.0 ** (torch.floor(torch.log2(t)) - 8)


def _within(got, ref, e):
    return bool(((got.detach().cpu().double() - ref).abs()
                 <= _hulp(ref.abs() + e) + e).all())


def _chain(N, C, H, W, strips):
    _, walkers, S, _ = ext.gn_plan(N, C, H, W, strips)
    strip = -(-H * W // S)
    return -(-strip // walkers) + walkers, S


def _per_c(t, Cg):
    return t.repeat_interleave(Cg, 1)[:, :, None, None]


class Ref:
    """float64 forward of one case and the bounds of the docstring."""

    def __init__(self, x, gam, bet, r, G, L):
        N, C, H, W = x.shape
        self.Cg, self.m, self.G = C // G, H * W * C // G, G
        xg = x.reshape(N, G, -1)
        self.mu = xg.sum(2) / self.m
        a = xg.abs().sum(2) / self.m
        q = (xg * xg).sum(2) / self.m
        var = (q - self.mu ** 2).clamp_min(0)
        self.inv = (var + EPS) ** -0.5
        self.dmu = L * U * a + U * self.mu.abs()
        dvar = L * U * (q + 2 * self.mu.abs() * a)
        self.dis = (dvar / 2 * ((var - dvar).clamp_min(0) + EPS) ** -1.5
                    + U * self.inv)
        mu, inv, dmu, dis = (_per_c(t, self.Cg) for t in
                             (self.mu, self.inv, self.dmu, self.dis))
        g, b = gam.view(1, C, 1, 1), bet.view(1, C, 1, 1)
        self.xc, self.xh = x - mu, (x - mu) * inv
        self.v = self.xh * g + b + (0 if r is None else r)
        ra = 0 if r is None else r.abs()
        self.e = 1.01 * (
            g.abs() * (self.xc.abs() * dis + (inv + dis) * dmu)
            + U * (g.abs() * (inv + dis) * (x.abs() + mu.abs()) + b.abs())
            + 2 * U * (self.v.abs() + ra))
        self.x, self.g, self.L = x, g, L
        self.c = (mu, inv, dmu, dis)

    def backward(self, ge):
        """(dx64, e_dx, dgamma64, e_dgamma, dbeta64, e_dbeta) for dy_eff."""
        mu, inv, dmu, dis = self.c
        x, g, L, m, xh, xc = self.x, self.g, self.L, self.m, self.xh, self.xc
        N, C = x.shape[:2]
        isb = inv + dis
        dxh = isb * dmu + xc.abs() * dis + 2 * U * xh.abs()
        A, B = ge.sum((2, 3)), (ge * xh).sum((2, 3))
        errA = L * U * ge.abs().sum((2, 3))
        errB = (ge.abs() * dxh).sum((2, 3)) + L * U * (ge * xh).abs().sum((2, 3))
        gv = g.view(1, C)

        def grp(t):
            return _per_c(t.reshape(N, self.G, self.Cg).sum(2), self.Cg)
        s1, s2 = grp(gv * A), grp(gv * B)
        ds1, ds2 = grp(gv.abs() * errA), grp(gv.abs() * errB)
        dx = g * inv * ge - inv / m * (s1 + xh * s2)
        k2x = -inv ** 2 * s2 / m * x
        k3 = -inv * s1 / m + inv ** 2 * mu * s2 / m
        e_dx = 1.01 * (
            (g * ge).abs() * dis
            + ((2 * inv * dis + dis ** 2) * s2.abs() * xc.abs()
               + isb ** 2 * ds2 * xc.abs()
               + isb ** 2 * (s2.abs() + ds2) * dmu) / m
            + (dis * s1.abs() + isb * ds1) / m
            + U * ((g * inv * ge).abs() + k2x.abs() + k3.abs())
            + 2 * U * ((k2x + k3).abs() + dx.abs()))
        db, dg = A.sum(0), B.sum(0)
        return (dx, e_dx, dg, errB.sum(0) + U * dg.abs(),
                db, errA.sum(0) + U * db.abs())


def _inputs(case, relu, resid):
    N, C, G, H, W, _ = case
    g = _gen(*case[:5], case[5] + 1, relu, resid)
    x = (torch.randn(N, C, H, W, generator=g, dtype=F64) * 1.5 + 0.7)
    dy = torch.randn(N, C, H, W, generator=g, dtype=F64)
    r = torch.randn(N, C, H, W, generator=g, dtype=F64) if resid else None
    sg = torch.randint(0, 2, (2, C), generator=g).to(F64) * 2 - 1
    gam = (sg[0] * (0.25 + torch.rand(C, generator=g, dtype=F64))).float()
    bet = (sg[1] * (0.5 + torch.rand(C, generator=g, dtype=F64))).float()
    rb = None if r is None else r.to(BF).double()
    return x.to(BF).double(), dy.to(BF).double(), rb, gam, bet


def _unpack(mask, N, C, H, W):
    bits = (mask.cpu().view(N, H, W, C // 8, 1)
            >> torch.arange(8, dtype=torch.uint8).view(1, 1, 1, 1, 8)) & 1
    return bits.reshape(N, H, W, C).permute(0, 3, 1, 2).bool()


@pytest.mark.parametrize("relu,resid", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("case", TABLE)
def test_random_data_within_the_rounding_bounds(case, relu, resid):
    N, C, G, H, W, strips = case
    x, dy, r, gam, bet = _inputs(case, relu, resid)
    L, S = _chain(N, C, H, W, strips)
    ref = Ref(x, gam.double(), bet.double(), r, G, L)
    n, f32 = N * C * H * W, torch.float32
    outs = [(n, BF), (N * S * 2 * C, f32), (N * G, f32), (N * 2 * C, f32)]
    _poison(*outs)
    rd = None if r is None else _dev(r)
    y, mean, invstd, mask = ext.gn_fwd(_dev(x), gam.to(DEV), bet.to(DEV), G,
                                       EPS, bool(relu), rd, True, strips)
    assert y.shape == x.shape and y.is_contiguous(memory_format=CL)
    if relu:
        bits = _unpack(mask, N, C, H, W)
        live = ref.v.abs() > ref.e
        assert (~live).sum().item() <= 1e-3 * n
        assert torch.equal(bits[live], (ref.v > 0)[live])
        ge = dy * bits
    else:
        assert mask.numel() == 0
        ge = dy
    dx64, e_dx, dg64, e_dg, db64, e_db = ref.backward(ge)
    _poison(*outs, (N * 3 * C, f32), (C, f32), (C, f32), (n, BF))
    out = ext.gn_bwd(_dev(x), _dev(dy), gam.to(DEV), mean, invstd, mask, G,
                     bool(relu), bool(resid), strips)
    assert len(out) == 3 + resid
    v = ref.v.clamp_min(0) if relu else ref.v
    assert _within(y, v, ref.e) and _within(out[0], dx64, e_dx)
    for got, want, e in ((mean, ref.mu, ref.dmu), (invstd, ref.inv, ref.dis),
                         (out[1], dg64, e_dg), (out[2], db64, e_db)):
        assert bool(((got.cpu().double() - want).abs() <= e).all())
    if resid:
        assert torch.equal(out[3].cpu().double(), ge)


def _exact_run(case, strips):
    N, C, G, H, W, _ = case
    g = _gen(9, *case[:5])
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    dy = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    gam = (torch.randint(0, 2, (C,), generator=g) * 2 - 1) \
        / (1.0 + torch.randint(0, 2, (C,), generator=g))
    bet = torch.randint(-3, 4, (C,), generator=g).float()
    m = H * W * C // G
    assert x.abs().reshape(N, G, -1).sum(2).max() < 2 ** 24
    assert dy.abs().sum((0, 2, 3)).max() < 2 ** 24
    _, mean, invstd, mask = ext.gn_fwd(_dev(x), gam.float().to(DEV),
                                       bet.to(DEV), G, EPS, False, None, True,
                                       strips)
    out = ext.gn_bwd(_dev(x), _dev(dy), gam.float().to(DEV), mean, invstd,
                     mask, G, False, False, strips)
    assert torch.equal(mean.cpu(), (x.reshape(N, G, -1).sum(2) / m).float())
    assert torch.equal(out[2].cpu().double(), dy.sum((0, 2, 3)))
    return mean, out[2]


@pytest.mark.parametrize("case", TABLE)
def test_exact_data_mean_and_dbeta_equal_float64(case):
    _exact_run(case, case[5])


def test_exact_data_is_the_same_at_any_strip_count():
    runs = [_exact_run(TABLE[2], s) for s in (1, 2, 3)]
    assert [ext.gn_plan(2, 16, 5, 5, s)[2] for s in (1, 2, 3)] == [1, 2, 3]
    for mean, db in runs[1:]:
        assert torch.equal(mean, runs[0][0]) and torch.equal(db, runs[0][1])


def test_gn_plan_is_shape_only_and_honours_strips():
    assert ext.gn_plan(2, 48, 6, 6, 2) == (6, 42, 2, 1)
    assert ext.gn_plan(1, 2056, 2, 2, 1) == (256, 1, 1, 2)
    assert ext.gn_plan(2, 8, 3, 7, 1000)[2] == 21        # clamped to rows
    slw, walkers, S, slices = ext.gn_plan(32, 256, 56, 56)
    assert (slw, walkers, slices) == (32, 8, 1) and 1 < S <= 64
    assert ext.gn_plan(32, 256, 56, 56, -1) == (slw, walkers, S, slices)


# via "module": the bare module; C = 12 takes the torch formula, fp32 sums in
# some order, so L = m.  via "conv_bn": behind a signed-permutation 1x1 conv,
# exact in bf16, so the float64 conv -> norm is the reference and the conv's
# dgrad of dx is exact; the conv's input is the residual too, so with bf16
# input the skip-gradient stash is armed and x.grad = dgrad(dx) + dresid comes
# out of the dgrad kernel, rounded once more.
@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("C,G,via", [(16, 4, "module"), (12, 3, "module"),
                                     (16, 4, "conv_bn")])
def test_layer_matches_the_float64_layer(C, G, via, dtype):
    N, H, W = 2, 5, 6
    TF = torch.nn.functional
    x, dy, r, gam, bet = _inputs((N, C, G, H, W, -1), 1, 1)
    gn = M_ops.GroupNorm(G, C, fuse_relu=True)
    assert list(gn.state_dict()) == ["weight", "bias"]
    with torch.no_grad():
        gn.weight.copy_(gam)
        gn.bias.copy_(bet)
    gn = gn.to(DEV)
    xd = x.to(dtype).contiguous(memory_format=CL).to(DEV).requires_grad_(True)
    L = H * W * C // G if C % 8 else _chain(N, C, H, W, -1)[0]
    if via == "conv_bn":
        w = torch.zeros(C, C, 1, 1, dtype=F64)
        w[torch.arange(C), torch.arange(C).flip(0), 0, 0] = \
            (1 - 2 * (torch.arange(C) % 2)).double()
        conv = M_ops.Conv2d(C, C, 1, bias=False)
        with torch.no_grad():
            conv.weight.copy_(w)
        y = F_ops.conv_bn(conv.to(DEV), gn, xd, residual=xd)
        xin, r = TF.conv2d(x, w), x
    else:
        rd = _dev(r).requires_grad_(True)
        y = gn(xd, residual=rd, pre_stats=None)
        xin = x
    y.backward(dy.to(y.dtype).to(DEV))
    ref = Ref(xin, gam.double(), bet.double(), r, G, L)
    assert bool((ref.v.abs() > ref.e).all())
    ge = dy * (ref.v > 0)
    dx64, e_dx, dg64, e_dg, db64, e_db = ref.backward(ge)
    assert xd.grad.dtype == dtype
    assert _within(y, ref.v.clamp_min(0), ref.e)
    assert bool(((gn.weight.grad.cpu().double() - dg64).abs() <= e_dg).all())
    assert bool(((gn.bias.grad.cpu().double() - db64).abs() <= e_db).all())
    if via == "conv_bn":
        e_in = TF.conv_transpose2d(_hulp(dx64.abs() + e_dx) + e_dx, w.abs())
        assert _within(xd.grad, TF.conv_transpose2d(dx64, w) + ge, e_in)
    else:
        assert _within(xd.grad, dx64, e_dx)
        assert torch.equal(rd.grad.cpu().double(), ge)


def test_converted_resnet_training_step_is_bitwise_repeatable():
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.parallel import convert_group_norm
    x = torch.randn(8, 3, 32, 32, generator=_gen(13)).to(DEV)
    t = torch.arange(8, device=DEV)
    runs = []
    try:
        for _ in range(2):
            amp._state.__init__()
            F_ops.clear_weight_cache()
            same_seeds(0)
            model = convert_group_norm(
                build_model("resnet18", num_classes=10, cifar_stem=True))
            assert not any(isinstance(m, M_ops.BatchNorm2d)
                           for m in model.modules())
            model = model.to(DEV).train()
            opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9,
                           nesterov=True)
            model, opt = amp.initialize(model, opt, opt_level="O1")
            opt.zero_grad()
            loss = F_ops.cross_entropy_loss(model(x), t) / 8
            with amp.scale_loss(loss, opt) as scaled:
                scaled.backward()
            opt.step()
            runs.append([loss.detach()] + [p.detach().clone()
                                           for p in model.parameters()])
    finally:
        amp._state.__init__()
    assert bool(runs[0][0].isfinite())
    for a, b in zip(*runs):
        assert torch.equal(a, b) and bool(a.isfinite().all())
