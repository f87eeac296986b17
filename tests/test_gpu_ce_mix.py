"""Mixed-target, smoothed cross-entropy kernels (``ce_mix_fwd`` /
``ce_mix_bwd``) against a float64 reference, with bounds derived from the
fp32 operation order of ``ops/hip/ce.hip`` — unit roundoff u = 2^-24 times
operation counts, the way ``test_gpu_norm_exact.py`` bounds the plain
kernels (its helpers are copied, not imported).

Target distribution of row i, with eps the fp32 value of the smoothing:
    q = eps/C + (1-eps) * (lam*onehot(a) + (1-lam)*onehot(b))
    rowloss = lse - pick,  pick = (1-eps)*(lam*x_a + (1-lam)*x_b)
                                  + (eps/C) * sum_c x_c

lse: the max / exp-sum part of both mix kernels is the plain kernels' code,
so e_lse is the plain bound (section 5 of test_gpu_norm_exact.py):
    per term of s, relative: u * ((mx - x_c) + 2*R_exp*K_exp + K_rnd)
    thread-per-row:  K_exp = 1,      K_rnd = C
    wave-per-row:    K_exp = E + 6,  K_rnd = 2E + 11,   E = 8*ceil(C/512)
    e_lse = e_s/s + 2*R_log*u*|log s| + u*|lse|

pick, with A = (1-eps)*(lam*|x_a| + (1-lam)*|x_b|), S = (eps/C)*sum|x_c|:
    the one-hot path rounds at: wb = fl(1-lam), the product, the sum of the
    two products, om = fl(1-eps), om*tsel, the final sum           -> 6
    the smoothing path: x_c passes D additions of the row sum, then
    ec = fl(eps/C), ec*sx, the final sum                           -> D + 3
      thread-per-row: D = C (one running sum)
      wave-per-row:   D = 3 + ceil(C/512) + 6 (pairwise tree over a chunk's
                      8 elements, one accumulator add per chunk of the lane,
                      6 shuffle levels; the chunk tree's 3 levels come on
                      top of the "chunks + 6" the accumulator alone gives)
    e_pick = u * (6*A + (D+3)*S)
    (a contracted multiply-add only removes a rounding)
    e_row  = e_lse + e_pick + u*|rowloss|
    e_loss = mean(e_row) + (ceil(B/256) + 9)*u*mean|rowloss|   (k_reduce_mean)

dlogits = fl(fl(p - q) * g), p = expf(fl(x - lse)), g = fl(dloss/B):
    q_c rounds at ec, wb, om, the product om*w, and two additions  -> 6
    e = g*(p*(e_lse + u*|x - lse| + 2*R_exp*u) + 6u*q + 3u*|p - q|) + 2^-125
sum_c dlogits is zero in exact arithmetic (sum q = 1); stored bf16 values
add a rounding each: |sum_c y_c| <= sum_c (e_c + 2^-8*(|ref_c| + e_c)).

With eps = 0, lam = 1, b = a the extra operations are exact (multiplications
by 1 and 0, additions of 0), so the result must sit inside the PLAIN bound
of the same reference, and within the sum of both bounds of ce_fwd/ce_bwd.
"""
import functools
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
F64 = torch.float64
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
R_EXP = 2           # measured by test_gpu_norm_exact.py, twice the maximum
R_LOG = 5
TINY = 2.0 ** -125
DLOSS = 0.37

CE_PATHS = [("bf16", 10), ("bf16", 63), ("fp32", 10),
            ("bf16", 64), ("bf16", 520), ("bf16", 1000)]
CE_BATCHES = [1, 5, 257]
SMOOTHINGS = [0.0, 0.1]


# ------------------------------------- helpers (test_gpu_norm_exact.py) ---

def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _cdiv(a, b):
    return -(-a // b)


def _bf(t64):
    return t64.float().to(BF).double()


def _assert_band(got, ref, e, what):
    lo, hi = _bf(ref - e), _bf(ref + e)
    bad = ~((got >= lo) & (got <= hi))      # a NaN is outside
    print(f"{what}: max |got - ref| {(got - ref).abs().max().item():.3e}, "
          f"max e {e.max().item():.3e}, outside {int(bad.sum())}")
    assert not bool(bad.any()), (what, int(bad.sum()),
                                 bad.nonzero()[:4].tolist())


def _assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}, "
          f"max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all()), (what, (err - bound).max().item())


def _ce_wave(dtype, C):
    return dtype == "bf16" and C % 8 == 0 and C >= 64


def _lse_bounds(x, wave):
    """lse and its bound: _ce_bounds of test_gpu_norm_exact.py"""
    B, C = x.shape
    mx = x.max(1, keepdim=True).values
    d = mx - x
    p = torch.exp(-d)
    s = p.sum(1)
    if wave:
        E = 8 * _cdiv(C // 8, 64)
        k_exp, k_rnd = E + 6, 2 * E + 11
    else:
        k_exp, k_rnd = 1, C
    e_s = U * SLACK * (p * (d + 2 * R_EXP * k_exp + k_rnd)).sum(1) + 1e-30
    lse = torch.log(s) + mx.squeeze(1)
    e_lse = (e_s / s * SLACK + 2 * R_LOG * U * torch.log(s).abs()
             + U * lse.abs()) * SLACK
    return lse, e_lse


def _mean_bound(row, e_row):
    B = row.shape[0]
    return e_row.mean() + (_cdiv(B, 256) + 9) * U * SLACK * row.abs().mean()


# -------------------------------------------------------------- the cases ---

@functools.lru_cache(maxsize=None)
def _case(dtype, C, B):
    """x as in test_gpu_norm_exact.py::_ce_case (overflow rows 2 and 4, the
    maximum in the last chunk in row 3); targets and weights placed by row."""
    x = torch.randn((B, C), generator=_gen((B, C), "ce x", dtype))
    if B > 2:
        x[2] *= 80.0                 # overflows without the max shift
    if B > 3:
        x[3, C - 1] = 30.0
    if B > 4:
        x[4] = x[4] * 80.0 - 80.0
    x = (x.to(BF) if dtype == "bf16" else x.float()).double()
    a = torch.randint(0, C, (B,), generator=_gen(B, C, "mix a"))
    b = torch.randint(0, C, (B,), generator=_gen(B, C, "mix b"))
    lam = torch.rand(B, generator=_gen(B, C, "mix lam"))
    a[0], b[0], lam[0] = 0, C - 1, 0.3        # generic lam, b in last chunk
    if B > 4:
        lam[1] = 0.0
        lam[2] = 1.0
        a[2] = int(x[2].argmax())
        lam[3] = 0.5
        a[3] = C - 1
        b[4] = a[4]                            # a == b, generic lam
    if B > 8:
        b[5], lam[5] = a[5], 0.0
        b[6], lam[6] = a[6], 1.0
        b[7] = (a[7] + 1) % C
        a[B - 1] = b[B - 1] = C - 1
    assert lam.dtype == torch.float32
    return x, a, b, lam


def _reference(x, a, b, lam, eps32, wave):
    B, C = x.shape
    lse, e_lse = _lse_bounds(x, wave)
    lam64 = lam.double()
    xa = x.gather(1, a.view(B, 1)).squeeze(1)
    xb = x.gather(1, b.view(B, 1)).squeeze(1)
    pick = ((1 - eps32) * (lam64 * xa + (1 - lam64) * xb)
            + eps32 / C * x.sum(1))
    A = (1 - eps32) * (lam64 * xa.abs() + (1 - lam64) * xb.abs())
    S = eps32 / C * x.abs().sum(1)
    D = 3 + _cdiv(C // 8, 64) + 6 if wave else C
    e_pick = U * SLACK * (6 * A + (D + 3) * S)
    row = lse - pick
    e_row = (e_lse + e_pick) * SLACK + U * SLACK * row.abs()
    q = torch.full((B, C), eps32 / C, dtype=F64)
    q += (1 - eps32) * (lam64.view(B, 1) * F.one_hot(a, C)
                        + (1 - lam64).view(B, 1) * F.one_hot(b, C))
    assert bool(((q.sum(1) - 1).abs() < 1e-12).all())
    return dict(lse=lse, e_lse=e_lse, row=row, e_row=e_row,
                loss=row.mean(), e_loss=_mean_bound(row, e_row), q=q)


def _dlogits_ref(x, r, q, q_roundings):
    B = x.shape[0]
    g = float(torch.tensor(DLOSS, dtype=torch.float32)) / B
    z = x - r["lse"].view(B, 1)
    p = torch.exp(z)
    ref = (p - q) * g
    e = g * SLACK * (p * (r["e_lse"].view(B, 1) + U * z.abs() + 2 * R_EXP * U)
                     + q_roundings * U * q + 3 * U * (p - q).abs()) + TINY
    return ref, e


def _check_dlogits(got, ref, e, bf16, what):
    if bf16:
        _assert_band(got, ref, e, what + " dlogits")
        half_ulp = 2.0 ** -8 * (ref.abs() + e)
    else:
        _assert_within(got, ref, e, what + " dlogits")
        half_ulp = torch.zeros_like(e)
    rowsum = got.sum(1).abs()
    bound = (e + half_ulp).sum(1)
    print(f"{what}: max |sum_c dlogits| {rowsum.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}")
    assert bool((rowsum <= bound).all()), what


def _dev(x, dtype):
    return x.to(BF if dtype == "bf16" else torch.float32).to(DEV)


def test_case_table_reaches_what_it_claims():
    for dtype, C in CE_PATHS:
        assert _ce_wave(dtype, C) == (C in (64, 520, 1000))
        x, a, b, lam = _case(dtype, C, 5)
        assert lam[1] == 0 and lam[2] == 1 and lam[3] == 0.5
        assert 0 < lam[0] < 1 and lam[0] != 0.5 and 0 < lam[4] < 1
        assert a[4] == b[4] and b[0] == C - 1 and a[3] == C - 1
        assert x[2].abs().max() > 88 and x[4].max() - x[4].min() > 88
        x, a, b, lam = _case(dtype, C, 257)
        assert a[5] == b[5] and a[6] == b[6] and a[7] != b[7]
        x, a, b, lam = _case(dtype, C, 1)
        assert b[0] == C - 1 and 0 < lam[0] < 1
    # 520 and 1000: a lane holds more than one chunk (the accumulator adds)
    assert _cdiv(1000 // 8, 64) == 2 and _cdiv(520 // 8, 64) == 2
    assert 257 % 4 == 1 and 257 % 256 == 1       # ragged wave- and row-block


@pytest.mark.parametrize("eps", SMOOTHINGS)
@pytest.mark.parametrize("B", CE_BATCHES)
@pytest.mark.parametrize("dtype,C", CE_PATHS)
def test_ce_mix(dtype, C, B, eps):
    x, a, b, lam = _case(dtype, C, B)
    wave = _ce_wave(dtype, C)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    r = _reference(x, a, b, lam, eps32, wave)
    xd, ad, bd, ld = _dev(x, dtype), a.to(DEV), b.to(DEV), lam.to(DEV)
    loss, lse = ext.ce_mix_fwd(xd, ad, bd, ld, eps)
    assert lse.shape == (B,) and lse.dtype == torch.float32
    assert loss.dim() == 0 and loss.dtype == torch.float32
    what = f"ce_mix {dtype} B={B} C={C} eps={eps}"
    _assert_within(lse.cpu().double(), r["lse"], r["e_lse"], what + " lse")
    _assert_within(loss.cpu().double(), r["loss"], r["e_loss"], what + " loss")

    dl = ext.ce_mix_bwd(xd, ad, bd, ld, lse, torch.tensor(DLOSS, device=DEV),
                        eps)
    assert dl.shape == (B, C) and dl.dtype == xd.dtype
    ref, e = _dlogits_ref(x, r, r["q"], 6)
    _check_dlogits(dl.cpu().double(), ref, e, dtype == "bf16", what)


@pytest.mark.parametrize("B", CE_BATCHES)
@pytest.mark.parametrize("dtype,C", CE_PATHS)
def test_hard_limit_sits_in_the_plain_bound(dtype, C, B):
    """eps = 0, lam = 1, b = a: inside the plain-CE bound of the same
    reference, and within the sum of both bounds of ce_fwd / ce_bwd."""
    x, a, _, _ = _case(dtype, C, B)
    wave = _ce_wave(dtype, C)
    lse_ref, e_lse = _lse_bounds(x, wave)
    row = lse_ref - x.gather(1, a.view(B, 1)).squeeze(1)
    e_row = e_lse + U * SLACK * row.abs()
    e_loss = _mean_bound(row, e_row)
    r = dict(lse=lse_ref, e_lse=e_lse)
    oh = F.one_hot(a, C).double()
    ref, e = _dlogits_ref(x, r, oh, 0)       # the plain kernel's one-hot is exact
    xd, ad = _dev(x, dtype), a.to(DEV)
    ones = torch.ones(B, device=DEV)
    dloss = torch.tensor(DLOSS, device=DEV)
    what = f"ce_mix->plain {dtype} B={B} C={C}"
    loss_m, lse_m = ext.ce_mix_fwd(xd, ad, ad, ones, 0.0)
    dl_m = ext.ce_mix_bwd(xd, ad, ad, ones, lse_m, dloss, 0.0)
    loss_p, lse_p = ext.ce_fwd(xd, ad)
    dl_p = ext.ce_bwd(xd, ad, lse_p, dloss)
    for name, (lm, lp) in (("mix", (loss_m, lse_m)), ("plain", (loss_p, lse_p))):
        _assert_within(lp.cpu().double(), lse_ref, e_lse, f"{what} {name} lse")
        _assert_within(lm.cpu().double(), row.mean(), e_loss,
                       f"{what} {name} loss")
    assert bool(((lse_m - lse_p).cpu().double().abs() <= 2 * e_lse).all())
    assert abs(float(loss_m) - float(loss_p)) <= 2 * float(e_loss)
    bf16 = dtype == "bf16"
    _check_dlogits(dl_m.cpu().double(), ref, e, bf16, what + " mix")
    _check_dlogits(dl_p.cpu().double(), ref, e, bf16, what + " plain")
    gap = (dl_m.double() - dl_p.double()).abs().cpu()
    half_ulp = 2.0 ** -8 * (ref.abs() + e) if bf16 else 0.0
    assert bool((gap <= 2 * (e + half_ulp)).all())
    print(f"{what}: bitwise equal to the plain kernels: "
          f"loss {torch.equal(loss_m, loss_p)}, lse {torch.equal(lse_m, lse_p)}, "
          f"dlogits {torch.equal(dl_m, dl_p)}")


# --------------------------------------------------- the public interface ---

@pytest.mark.parametrize("dtype,C", [("bf16", 10), ("fp32", 10), ("bf16", 64)])
def test_default_dispatch_is_the_plain_path(dtype, C, monkeypatch):
    from ddp_tricks_amd.ops import functional as Fn

    def _never(*a, **k):
        raise AssertionError("a hard target without smoothing reached the "
                             "mixed-target Function")

    monkeypatch.setattr(Fn._HIPMixCrossEntropy, "apply", _never)
    x, a, _, _ = _case(dtype, C, 5)
    xd, ad = _dev(x, dtype), a.to(DEV)
    xg = xd.clone().requires_grad_(True)
    loss = Fn.cross_entropy_loss(xg, ad)
    loss.backward()
    loss_k, lse_k = ext.ce_fwd(xd, ad)
    dl_k = ext.ce_bwd(xd, ad, lse_k, torch.ones((), device=DEV))
    assert torch.equal(loss.detach(), loss_k)
    assert torch.equal(xg.grad, dl_k)
    loss0 = Fn.cross_entropy_loss(xd, ad, label_smoothing=0.0)
    assert torch.equal(loss0, loss_k)


@pytest.mark.parametrize("dtype,C", [("bf16", 10), ("fp32", 10), ("bf16", 520)])
def test_autograd_mixed_target(dtype, C):
    from ddp_tricks_amd.ops import MixedTarget, cross_entropy_loss
    x, a, b, lam = _case(dtype, C, 5)
    xd, ad, bd, ld = _dev(x, dtype), a.to(DEV), b.to(DEV), lam.to(DEV)
    mt = MixedTarget(a, b, lam.double()).to(DEV)
    assert mt.a.is_cuda and mt.lam.dtype == torch.float32
    assert torch.equal(mt.dominant().cpu(), torch.where(lam >= 0.5, a, b))
    xg = xd.clone().requires_grad_(True)
    loss = cross_entropy_loss(xg, mt, 0.1)
    (loss * 3.0).backward()
    loss_k, lse_k = ext.ce_mix_fwd(xd, ad, bd, ld, 0.1)
    dl_k = ext.ce_mix_bwd(xd, ad, bd, ld, lse_k,
                          torch.full((), 3.0, device=DEV), 0.1)
    assert torch.equal(loss.detach(), loss_k) and torch.equal(xg.grad, dl_k)
    # a tensor target with smoothing: b = a, lam = 1
    xg = xd.clone().requires_grad_(True)
    cross_entropy_loss(xg, ad, 0.1).backward()
    ones = torch.ones(5, device=DEV)
    loss_k, lse_k = ext.ce_mix_fwd(xd, ad, ad, ones, 0.1)
    assert torch.equal(
        xg.grad, ext.ce_mix_bwd(xd, ad, ad, ones, lse_k,
                                torch.ones((), device=DEV), 0.1))
    # a MixedTarget without smoothing goes to the mix kernels as well
    l0 = cross_entropy_loss(xd, mt)
    assert torch.equal(l0, ext.ce_mix_fwd(xd, ad, bd, ld, 0.0)[0])


def test_host_checks():
    x, a, b, lam = _case("bf16", 10, 5)
    xd, ad, bd, ld = _dev(x, "bf16"), a.to(DEV), b.to(DEV), lam.to(DEV)
    lse = torch.zeros(5, device=DEV)
    dloss = torch.ones((), device=DEV)
    bad = [
        (xd, ad.int(), bd, ld, 0.1), (xd, ad, bd.int(), ld, 0.1),
        (xd, ad, bd, ld.double(), 0.1), (xd, ad[:4], bd, ld, 0.1),
        (xd, ad, bd, ld[:4], 0.1), (xd, ad, b, ld, 0.1),
        (xd, ad, bd, lam, 0.1), (xd, a, bd, ld, 0.1),
        (xd, ad, bd, ld, 1.0), (xd, ad, bd, ld, -0.01),
        (xd.half(), ad, bd, ld, 0.1),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.ce_mix_fwd(*args)
        with pytest.raises(RuntimeError):
            ext.ce_mix_bwd(*args[:4], lse, dloss, args[4])
