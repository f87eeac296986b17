"""Squeeze-and-Excitation kernels (ops/hip/se.hip) and the junction built on
them, against float64 on the CPU over the same bf16-rounded operands.

u = 2^-24, hulp(t) = 2^(floor(log2 t) - 8) (half a bf16 ulp), HW = H W.
Bounds are first order; the factor 1.05 covers the dropped products of two
relative errors (each < 2^-6 here).
* Gate: __expf(x) = exp2(fl(x log2 e)): the product's rounding moves the
  exponent by <= 11.6 u for |x| <= 8, i.e. 8.1 u relative in the result; the
  exp2 instruction adds 1 ulp (2 u), the add and the divide u each:
  |s - s64| <= ds = 13 u s64.
* y = bf16(fma(u, s, r)): e = |u| ds + u |v64|, |y - y64| <= hulp(|v64| + e)
  + e; the mask equals v64 > 0 wherever |v64| > e.
* da = bf16(t s (1 - s)), t = sum g u by fma: a lane adds L = ceil(strip /
  walkers) terms, the join `walkers`, the gate kernel S strips:
  et = (L + walkers + S) u sum|g u|;  e = et s(1-s) + |t| (ds + u) + 2 u |da64|.
* dx = bf16(fma(g, s, q)), q = fl(dz / HW): e = |g| ds + u |q| + u |dx64|.
* Junction (derived, not measured): bf16 roundings at z, h, a, da, dh, dz,
  each <= 2^-8 relative (half an ulp of an 8-bit significand), carried
  through |W| and the gate's derivatives, plus (K + 2) u sum|terms| for each
  fp32 contraction of length K; see _junction.  Largest error / bound seen
  on an MI355X: y 0.985, dx 0.90 (both are the output's own bf16 rounding),
  parameter gradients 0.41.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

U, R8 = 2.0 ** -24, 2.0 ** -8
BF, F64, CL = torch.bfloat16, torch.float64, torch.channels_last
EPI = [(0, 0), (1, 0), (1, 1)]          # (relu, residual)

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import SqueezeExcite, load_extension
    from ddp_tricks_amd.ops import modules as M_ops
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

# (N, C, H, W, strips): one row, one chunk; slw 3, an idle lane, fewer rows
# than walkers; 5 walkers of 8 chunks; a second slice with one live chunk;
# four strips with a ragged last one (combine path); strips capped at 81 rows
EXACT = [(2, 8, 1, 1, -1), (2, 24, 7, 7, -1), (3, 64, 5, 3, -1),
         (2, 2056, 3, 3, -1), (2, 32, 9, 9, 4), (2, 32, 9, 9, 1000)]


def _gen(*tag):
    return torch.Generator().manual_seed(hash(tag) % 2 ** 31)


def _dev(t64):
    t = t64.to(BF)
    return (t.contiguous(memory_format=CL) if t.dim() == 4 else t).to(DEV)


def _hulp(t):
    return 2.0 ** (torch.floor(torch.log2(t)) - 8)


def _ratio(got, ref, e):
    """largest |got - ref| / (hulp(|ref| + e) + e); <= 1 passes"""
    err = (got.detach().cpu().double() - ref).abs()
    return float((err / (_hulp(ref.abs() + e + 1e-300) + e + 1e-300)).max())


def _unpack(mask, N, C, H, W):
    bits = (mask.cpu().view(N, H, W, C // 8, 1)
            >> torch.arange(8, dtype=torch.uint8).view(1, 1, 1, 1, 8)) & 1
    return bits.reshape(N, H, W, C).permute(0, 3, 1, 2).bool()


def _nc(t):
    return t[:, :, None, None]


def _rnd(g, *s, k=1.0):
    return (torch.randn(*s, generator=g, dtype=F64) * k).to(BF).double()


@pytest.mark.parametrize("relu,resid", EPI)
@pytest.mark.parametrize("case", EXACT)
def test_exact_data_equals_float64(case, relu, resid):
    N, C, H, W, strips = case
    HW, g = H * W, _gen(*case, relu, resid)
    u = torch.randint(-4, 5, (N, C, H, W), generator=g).to(F64) / 2
    r = torch.randint(-3, 4, (N, C, H, W), generator=g).to(F64) if resid else None
    dy = torch.randint(-2, 3, (N, C, H, W), generator=g).to(F64)
    dz = torch.randint(-2, 3, (N, C), generator=g).to(F64) * HW
    assert torch.equal(dz.to(BF).double(), dz)
    ud, dyd, a = _dev(u), _dev(dy), torch.zeros(N, C, dtype=BF, device=DEV)
    z = ext.se_squeeze(ud, strips)
    assert torch.equal(z.cpu(), (u.sum((2, 3)) / HW).float().to(BF))
    y, mask = ext.se_apply(ud, a, None if r is None else _dev(r), bool(relu),
                           True)
    v = u * 0.5 + (0 if r is None else r)
    assert y.is_contiguous(memory_format=CL)
    assert torch.equal(y.cpu().double(), v.clamp_min(0) if relu else v)
    if relu:
        assert mask.shape == (N * HW, C // 8)
        assert torch.equal(_unpack(mask, N, C, H, W), v > 0)
    else:
        assert mask.numel() == 0
    ge = dy * (v > 0) if relu else dy
    da = ext.se_bwd_gate(dyd, ud, mask, a, bool(relu), strips)
    assert torch.equal(da.cpu(), ((ge * u).sum((2, 3)) * 0.25).float().to(BF))
    dx, dres = ext.se_bwd_dx(dyd, ud, mask, a, _dev(dz), bool(relu),
                             bool(resid) or not relu)
    assert torch.equal(dx.cpu().double(), ge * 0.5 + _nc(dz) / HW)
    if not relu:        # the plain epilogue hands dy back, writes nothing
        assert dres.data_ptr() == dyd.data_ptr()
    else:
        assert (dres is None) if not resid else \
            torch.equal(dres.cpu().double(), ge)


@pytest.mark.parametrize("relu,resid", EPI)
@pytest.mark.parametrize("case", [(2, 40, 9, 7, -1), (3, 264, 6, 6, 3)])
def test_random_data_within_the_rounding_bounds(case, relu, resid):
    N, C, H, W, strips = case
    HW, g, n = H * W, _gen(*case, relu, resid), N * C * H * W
    u, dy, dz = _rnd(g, N, C, H, W), _rnd(g, N, C, H, W), _rnd(g, N, C)
    r = _rnd(g, N, C, H, W) if resid else None
    a = ((torch.rand(N, C, generator=g, dtype=F64) * 16 - 8).to(BF).double())
    s = 1 / (1 + torch.exp(-a))
    ds = 13 * U * s
    v = u * _nc(s) + (0 if r is None else r)
    e = 1.05 * (u.abs() * _nc(ds) + U * v.abs())
    y, mask = ext.se_apply(_dev(u), _dev(a), None if r is None else _dev(r),
                           bool(relu), True)
    ge = dy
    if relu:
        bits, live = _unpack(mask, N, C, H, W), v.abs() > e
        assert (~live).sum().item() <= 1e-3 * n
        assert torch.equal(bits[live], (v > 0)[live])
        ge = dy * bits
    _, walkers, S, _ = ext.se_plan(N, C, H, W, strips)
    L = -(-(-(-HW // S)) // walkers)
    t = (ge * u).sum((2, 3))
    et = (L + walkers + S) * U * (ge * u).abs().sum((2, 3))
    da64 = t * s * (1 - s)
    e_da = 1.05 * (et * s * (1 - s) + t.abs() * (ds + U) + 2 * U * da64.abs())
    dx64 = ge * _nc(s) + _nc(dz) / HW
    e_dx = 1.05 * (ge.abs() * _nc(ds) + U * _nc(dz.abs()) / HW + U * dx64.abs())
    da = ext.se_bwd_gate(_dev(dy), _dev(u), mask, _dev(a), bool(relu), strips)
    dx, _ = ext.se_bwd_dx(_dev(dy), _dev(u), mask, _dev(a), _dev(dz),
                          bool(relu), bool(resid))
    ratios = (_ratio(y, v.clamp_min(0) if relu else v, e),
              _ratio(da, da64, e_da), _ratio(dx, dx64, e_dx))
    print("error / bound (y, da, dx):", ratios)
    assert max(ratios) <= 1


def _junction(u, r, dy, w1, b1, w2, b2, relu):
    """float64 junction and first-order bounds: ((y, e_y), live, [(grad,
    bound)] for u, fc1.w, fc1.b, fc2.w, fc2.b), g).  `live` marks where the
    relu's sign is decided beyond e_y; the caller zeroes dy elsewhere."""
    HW = u.shape[2] * u.shape[3]

    def mm(x, ex, w, ew=0):     # x @ w with errors ex, ew and fp32 sums
        return (ex @ w.abs() + x.abs() @ (ew + (x.shape[1] + 2) * U * w.abs()))
    z = u.mean((2, 3))
    ez = R8 * z.abs()
    hp = z @ w1.T + b1
    eh = mm(z, ez, w1.T) + R8 * hp.abs()
    assert bool((hp.abs() > eh).all())
    h, hm = hp.clamp_min(0), hp > 0
    a = h @ w2.T + b2
    ea = mm(h, eh * hm, w2.T) + R8 * a.abs()
    s = 1 / (1 + torch.exp(-a))
    es = 1.05 * s * (1 - s) * ea + 13 * U * s
    v = u * _nc(s) + (0 if r is None else r)
    ey = 1.05 * (u.abs() * _nc(es) + U * v.abs())
    live = (v.abs() > ey) if relu else torch.ones_like(v, dtype=torch.bool)
    g = dy * live * ((v > 0) if relu else 1)
    t = (g * u).sum((2, 3))
    da = t * s * (1 - s)
    eda = 1.05 * (t.abs() * (1 - 2 * s).abs() * es
                  + (HW + 2) * U * (g * u).abs().sum((2, 3))) + R8 * da.abs()
    dhl = da @ w2
    edh = (mm(da, eda, w2) + R8 * dhl.abs()) * hm
    dh = dhl * hm
    dz = dh @ w1
    edz = mm(dh, edh, w1) + R8 * dz.abs()
    dx = g * _nc(s) + _nc(dz) / HW
    edx = 1.05 * (g.abs() * _nc(es) + _nc(edz) / HW + 2 * U * dx.abs())
    grads = [(dx, edx), (dh.T @ z, 1.05 * mm(dh.T, edh.T, z, ez)),
             (dh.sum(0), edh.sum(0) + 6 * U * dh.abs().sum(0)),
             (da.T @ h, 1.05 * mm(da.T, eda.T, h, eh * hm)),
             (da.sum(0), eda.sum(0) + 6 * U * da.abs().sum(0))]
    return (v.clamp_min(0) if relu else v, ey), live, grads, g


@pytest.mark.parametrize("relu,via", [(1, "module"), (0, "module"),
                                      (1, "conv")])
def test_junction_matches_the_float64_composition(relu, via):
    N, C, H = 4, 64, 6
    g = _gen(7, relu, len(via))
    x, dy = _rnd(g, N, C, H, H), _rnd(g, N, C, H, H)
    ps = [_rnd(g, 4, C, k=0.5), _rnd(g, 4), _rnd(g, C, 4), _rnd(g, C)]
    se = SqueezeExcite(C, reduction=16)
    with torch.no_grad():
        for p, v in zip(se.parameters(), ps):
            p.copy_(v.view(p.shape))
    se = se.to(DEV)
    xd = _dev(x).requires_grad_(True)
    u, r, rd = x, (x.flip(0) if relu else None), None
    if via == "conv":           # exact signed-permutation 1x1 conv in front:
        w = torch.zeros(C, C, 1, 1, dtype=F64)      # x is input and residual
        w[torch.arange(C), torch.arange(C).flip(0), 0, 0] = \
            (1 - 2 * (torch.arange(C) % 2)).double()
        conv = M_ops.Conv2d(C, C, 1, bias=False)
        with torch.no_grad():
            conv.weight.copy_(w)
        u, r = torch.nn.functional.conv2d(x, w), x
        y = se(conv.to(DEV)(xd), residual=xd, fuse_relu=True)
    else:
        rd = None if r is None else _dev(r).requires_grad_(True)
        y = se(xd, residual=rd, fuse_relu=bool(relu))
    (y64, ey), live, grads, ge = _junction(u, r, dy, *ps, relu)
    assert (~live).sum().item() <= 1e-2 * live.numel()
    y.backward(_dev(dy * live))
    rf = _ratio(y, y64, ey)
    got = [xd.grad] + [p.grad.flatten(1) if p.dim() == 4 else p.grad
                       for p in se.parameters()]
    if via == "conv":   # dresid rode the stash into the conv's dgrad epilogue
        assert xd._ddpx_skipbox == {}
        TF, (dx, edx) = torch.nn.functional, grads[0]
        grads[0] = (TF.conv_transpose2d(dx, w) + ge,
                    TF.conv_transpose2d(_hulp(dx.abs() + edx) + edx, w.abs()))
    elif relu:
        assert torch.equal(rd.grad.cpu().double(), ge)
    rg = [_ratio(a, ref, e) if i == 0 else
          float(((a.cpu().double() - ref).abs() / (e + 1e-300)).max())
          for i, (a, (ref, e)) in enumerate(zip(got, grads))]
    print("error / bound: forward", rf, "gradients", rg)
    assert rf <= 1 and max(rg) <= 1


def test_se_plan_is_shape_only():
    assert ext.se_plan(2, 24, 7, 7) == (3, 85, 1, 1)
    assert ext.se_plan(2, 32, 9, 9, 1000) == (4, 64, 81, 1)
    slw, walkers, S, slices = ext.se_plan(32, 2048, 7, 7)
    assert (slw, walkers, slices) == (256, 1, 1) and 1 < S <= 64


_STEP = """
import hashlib, torch
from ddp_tricks_amd import amp, same_seeds
from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.ops import functional as F
from ddp_tricks_amd.ops.optim import FusedSGD
same_seeds(0)
dev = torch.device("cuda:0")
model = build_model("se_resnext50_32x4d", num_classes=10,
                    cifar_stem=True).to(dev).train()
opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
model, opt = amp.initialize(model, opt, opt_level="O1")
x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev)
opt.zero_grad()
loss = F.cross_entropy_loss(model(x), torch.arange(4, device=dev)) / 4
with amp.scale_loss(loss, opt) as scaled:
    scaled.backward()
opt.step()
d = hashlib.sha256(loss.detach().cpu().numpy().tobytes())
for p in model.parameters():
    d.update(p.detach().cpu().numpy().tobytes())
assert bool(loss.isfinite())
print("DIGEST", d.hexdigest(), float(loss))
"""


def test_se_resnext_amp_step_is_bitwise_equal_in_two_processes():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for _ in range(2):
        p = subprocess.run([sys.executable, "-c", _STEP], cwd=root,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append([ln for ln in p.stdout.splitlines()
                     if ln.startswith("DIGEST")][-1])
    assert outs[0] == outs[1] and len(outs[0].split()[1]) == 64
