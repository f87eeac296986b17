"""GPU tier of FusedLAMB: the tick, moments + pair-square-sum, per-tensor
ratio and step kernels behind ``ext.fused_lamb`` and the optimizer on top
of them.  Shapes and packing as in tests/test_gpu_lars.py, including the
tensor of 257 chunks + 3 elements (more chunks than the ratio kernel's
block has threads)."""
import pytest
import torch

from test_gpu_adamw import (NCOEF, _counters, adam_moments_ref, amp_run,
                            coef_ref, lazy_clip_check, overflow_check,
                            same_step, twice_check)
from test_gpu_lars import (CASES, CH, GUARD, MULTI, U, _buffers, _ext,
                           _guards_intact, _nchunks, _pack, _param_views,
                           _randn, _set_grads, _spread)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


# ------------------------------------------------------ 1. exact first step ---

@pytest.mark.parametrize("gs", [None, 0.5])
@pytest.mark.parametrize("case", list(CASES))
def test_exact_first_step(case, gs):
    """betas = (0.5, 0.75), eps = 1, wd = 0, m = v = 0 and the (scaled)
    gradient is +-1 at 4**k spread positions, 0 elsewhere: m = g/2,
    v = g*g/4, bc1 = 1/2, bc2 = 1/4, so u = (+-1)/(1 + 1) = +-1/2 there and
    0/(0 + 1) = 0 elsewhere, |u| = 2**(k-1).  p holds +-2**(1 + i%5) at
    4**k positions, |p| = 2**(1 + i%5 + k): every partial and total is an
    integer multiple of 1/4 far below 2**24, exact in any order, and the
    ratio 2**(2 + i%5) must come out exactly.  It differs between
    neighbouring tensors, so a ratio or a coefficient at a
    launch-group-local index shows.  lr = 2**-6: p - lr*r*u is exact."""
    ext = _ext()
    sizes, lead = CASES[case]
    lr = 2.0 ** -6
    ps, gs_, want_r = [], [], []
    for i, n in enumerate(sizes):
        p, _ = _spread(n, 2.0 ** (1 + i % 5), 100 + i)
        g, _ = _spread(n, 1.0 / (gs or 1.0), 200 + i)
        ps.append(p)
        gs_.append(g)
        want_r.append(1.0 if n == 0 else 2.0 ** (2 + i % 5))
    zeros = [torch.zeros(n) for n in sizes]
    coef = None if gs is None else torch.tensor([gs], device=DEV)
    pv, fp, gp = _pack(ps, lead)
    gv, fg, gg = _pack(gs_, (lead + 1) % 4)
    mv, fm, gm = _pack(zeros, (lead + 2) % 4)
    vv, fv, gvv = _pack(zeros, (lead + 3) % 4)
    fg_before = fg.clone()
    n = len(sizes)
    steps, coefs = _counters(n)
    partials, ratios = _buffers(sizes)
    ext.fused_lamb(pv, gv, mv, vv, steps, coefs, partials, ratios, lr, 0.5,
                   0.75, 1.0, 0.0, False, 10.0, None, coef)
    assert ratios.cpu()[:n].tolist() == want_r        # exact, global index
    assert bool((ratios.cpu()[n:] == GUARD).all())
    assert steps.cpu()[:n].tolist() == [1.0] * n
    assert bool((steps.cpu()[n:] == GUARD).all())
    want_c = torch.tensor([2 * lr, 0.5, 0.5, 0.25] * n)
    assert torch.equal(coefs.cpu()[:NCOEF * n], want_c)
    assert bool((coefs.cpu()[NCOEF * n:] == GUARD).all())
    nc = _nchunks(sizes)
    assert bool((partials.cpu()[2 * nc:] == GUARD).all())
    assert torch.equal(fg, fg_before)                 # gradients kept
    for i in range(n):
        ge = gs_[i] * (gs or 1.0)                     # +-1 or 0
        assert torch.equal(mv[i].cpu(), 0.5 * ge), i
        assert torch.equal(vv[i].cpu(), 0.25 * ge * ge), i
        want_p = ps[i] - lr * want_r[i] * 0.5 * ge
        assert torch.equal(pv[i].cpu(), want_p), i
    assert _guards_intact(fp, gp) and _guards_intact(fm, gm)
    assert _guards_intact(fv, gvv) and _guards_intact(fg, gg)

    # trust_clip: the same step with every ratio cut to max_trust = 2
    p2, fp2, gp2 = _pack(ps, lead)
    m2, _, _ = _pack(zeros, (lead + 2) % 4)
    v2, _, _ = _pack(zeros, (lead + 3) % 4)
    steps2, coefs2 = _counters(n)
    ext.fused_lamb(p2, gv, m2, v2, steps2, coefs2, partials, ratios, lr, 0.5,
                   0.75, 1.0, 0.0, True, 2.0, None, coef)
    assert ratios.cpu()[:n].tolist() == [min(r, 2.0) for r in want_r]
    for i in range(n):
        ge = gs_[i] * (gs or 1.0)
        want_p = ps[i] - lr * min(want_r[i], 2.0) * 0.5 * ge
        assert torch.equal(p2[i].cpu(), want_p), i
    assert _guards_intact(fp2, gp2)


def test_buffers_too_small_is_an_error():
    ext = _ext()
    t = [torch.ones(CH + 1), torch.ones(3)]           # 3 chunks
    pv, fp, _ = _pack(t, 0)
    gv, _, _ = _pack(t, 1)
    mv, _, _ = _pack(t, 2)
    vv, _, _ = _pack(t, 3)
    before = fp.clone()
    steps, coefs = torch.zeros(2, device=DEV), torch.zeros(8, device=DEV)
    ok_p, ok_r = torch.zeros(6, device=DEV), torch.zeros(2, device=DEV)
    tail = (1e-3, 0.9, 0.999, 1e-6, 0.01, False, 10.0, None, None)
    with pytest.raises(RuntimeError, match="partials"):
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs,
                       torch.zeros(5, device=DEV), ok_r, *tail)
    with pytest.raises(RuntimeError, match="ratios"):
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs, ok_p,
                       torch.zeros(1, device=DEV), *tail)
    with pytest.raises(RuntimeError, match="steps"):
        ext.fused_lamb(pv, gv, mv, vv, steps[:1], coefs, ok_p, ok_r, *tail)
    with pytest.raises(RuntimeError, match="coefs"):
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs[:7], ok_p, ok_r, *tail)
    with pytest.raises(RuntimeError):                 # grad of another size
        ext.fused_lamb(pv, gv[::-1], mv, vv, steps, coefs, ok_p, ok_r, *tail)
    assert torch.equal(fp, before)
    assert steps.tolist() == [0.0, 0.0]


# ----------------------------------------------------------- 2. random data ---

def _random_cases():
    out = []
    for case in MULTI:
        cfgs = [(0.0, False), (0.05, False), (0.05, True)]
        if case == "wide":
            cfgs = cfgs[1:2]
        out += [(case,) + c for c in cfgs]
    return out


@pytest.mark.parametrize("case,wd,trust_clip", _random_cases())
def test_random_matches_float64(case, wd, trust_clip):
    """Three steps (two for the wide tensor) against the documented formula
    in float64, each step's reference started from the state the kernel
    left.  The second step's gradients hold a zero tensor and scattered
    zeros.  U = 2**-24, first-order terms, constants are doubles rounded to
    fp32 once; the moments as in tests/test_gpu_adamw.py (|m - m_ref| <=
    3U*M, v relative 4U).

    Direction.  mh = m / bc1: (3U*M + 2U*|m|)/bc1 <= 5U*M/bc1.
    vh = v / bc2: 4U + 2U = 6U;  s = sqrt(vh): 3U + U = 4U;  d = s + eps,
    positive terms: 5U.  q = mh / d: 5U*Q + 5U*Q + U*Q = 11U*Q with
    Q = (M/bc1)/d.  u = fma(wd, p, q): U*wd|p| (constant) + U*(Q + wd|p|):
        |u - u_ref| <= U*(12Q + 2wd|p|) <= 12U*A,   A = Q + wd|p|.

    Ratio.  A chunk's sum of squares is <= 64 sequential fmaf terms per
    thread plus an 8-level tree over positive terms, relative <= 72U, half
    of it on a norm (the figure of tests/test_gpu_lars.py); the double sums
    add nothing at this scale.  |p| carries 36U.  |u| carries 36U and the
    element errors above: | |u| - |u_ref| | <= |u - u_ref| <= 12U*|A|, that
    is 12U*kappa relative with kappa = |A|_2 / |u_ref|_2 >= 1, a condition
    number taken from the reference.  One final rounding:
        ratio relative <= RHO = U*(73 + 12*kappa)
    min(., max_trust) is 1-Lipschitz, so the clipped ratio is within
    RHO * r_ref (r_ref before the clip); where that exceeds RHO * max_trust
    by more than a second-order term, both sides are clipped and equal.

    Step.  a = lr*r with lr rounded and one product rounding: RHO + 2U.
    p = fma(-a, u, p):
        (RHO + 2U)*lr*r*|u_ref| + lr*r*12U*A + U*(|p| + lr*r*A)
        <= (RHO + 2U)*lr*r*|u_ref| + U*(|p| + 13*lr*r*A)
    asserted with U*(2|p| + 14*lr*r*A) for the second-order remainder, r
    the reference's ratio after the clip plus its error bound."""
    ext = _ext()
    sizes, lead = CASES[case]
    lr, b1, b2, eps, max_trust = 1e-2, 0.9, 0.999, 1e-6, 1.5
    n = len(sizes)
    pv, fp, gp = _pack(_randn(sizes, 21), lead)
    mv, fm, gm = _pack([torch.zeros(k) for k in sizes], (lead + 2) % 4)
    vv, fv, gvv = _pack([torch.zeros(k) for k in sizes], (lead + 3) % 4)
    steps, coefs = _counters(n)
    partials, ratios = _buffers(sizes)
    worst_r = worst_p = 0.0
    for step in (1, 2, 3)[:2 if case == "wide" else 3]:
        g0 = _randn(sizes, 30 + step, scale=3.0)
        if step == 2:
            if n > 1:
                g0[1].zero_()
            for g in g0:
                g[::3] = 0
        gv, fg, gg = _pack(g0, (lead + 1) % 4)
        before = [[t.cpu().double() for t in lst] for lst in (pv, mv, vv)]
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs, partials, ratios, lr,
                       b1, b2, eps, wd, trust_clip, max_trust, None, None)
        assert steps.cpu()[:n].tolist() == [float(step)] * n
        got_r = ratios.cpu()[:n].double()
        _, _, bc1, bc2 = coef_ref(lr, b1, b2, step)
        for i in range(n):
            p, m, v = (before[k][i] for k in range(3))
            g = g0[i].double()
            m_ref, v_ref, M = adam_moments_ref(g, m, v, b1, b2)
            assert bool(((mv[i].cpu().double() - m_ref).abs()
                         <= 4 * U * M).all()), (step, i)
            assert bool(((vv[i].cpu().double() - v_ref).abs()
                         <= 5 * U * v_ref).all()), (step, i)
            d = (v_ref / bc2).sqrt() + eps
            u_ref = (m_ref / bc1) / d + wd * p
            A = (M / bc1) / d + wd * p.abs()
            wn, un = float(p.norm()), float(u_ref.norm())
            if not (wn > 0 and un > 0):
                assert float(got_r[i]) == 1.0, (step, i)
                r, rho = 1.0, 0.0
            else:
                r = wn / un
                rho = U * (73 + 12 * float(A.norm()) / un)
                err_r = abs(float(got_r[i])
                            - (min(r, max_trust) if trust_clip else r))
                worst_r = max(worst_r, err_r / (rho * r))
                assert err_r <= rho * r, (step, i)
                if trust_clip:
                    r = min(r, max_trust)
            if sizes[i] == 0:
                continue
            p_ref = p - lr * r * u_ref
            r_hi = r * (1 + rho)
            bound = ((rho + 2 * U) * lr * r_hi * u_ref.abs()
                     + U * (2 * p.abs() + 14 * lr * r_hi * A))
            err = (pv[i].cpu().double() - p_ref).abs()
            worst_p = max(worst_p, float((err / bound).max()))
            assert bool((err <= bound).all()), (step, i)
        assert _guards_intact(fg, gg)
    print(f"{case} wd={wd} clip={trust_clip}: ratio err/bound max "
          f"{worst_r:.3f}, p err/bound max {worst_p:.3f}")
    assert _guards_intact(fp, gp) and _guards_intact(fm, gm)
    assert _guards_intact(fv, gvv)
    assert bool((ratios.cpu()[n:] == GUARD).all())
    assert bool((partials.cpu()[2 * _nchunks(sizes):] == GUARD).all())


def test_degenerate_tensors():
    """A zero gradient from zero moments gives u = wd*p (ratio 1/wd); with
    wd = 0 too, |u| = 0 and the ratio is 1; an all-zero parameter gets
    ratio 1; a zero-size tensor between others changes nothing for its
    neighbours; nothing becomes non-finite."""
    ext = _ext()
    sizes = [7, CH + 1, 0, 5, 9]
    p0 = _randn(sizes, 31)
    g0 = _randn(sizes, 32)
    g0[1].zero_()
    p0[3].zero_()

    def run(keep, wd):
        pv, fp, gp = _pack([p0[i] for i in keep], 1)
        gv, _, _ = _pack([g0[i] for i in keep], 2)
        mv, fm, gm = _pack([torch.zeros(sizes[i]) for i in keep], 3)
        vv, fv, _ = _pack([torch.zeros(sizes[i]) for i in keep], 0)
        ks = [sizes[i] for i in keep]
        steps, coefs = _counters(len(keep))
        partials, ratios = _buffers(ks)
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs, partials, ratios, 1e-2,
                       0.9, 0.999, 1e-6, wd, False, 10.0, None, None)
        assert _guards_intact(fp, gp) and _guards_intact(fm, gm)
        for f in (fp, fm, fv):
            assert bool(torch.isfinite(f).all())
        return [v.cpu() for v in pv], ratios.cpu()[:len(keep)]

    p_all, r_all = run([0, 1, 2, 3, 4], 0.0)
    assert r_all[1:4].tolist() == [1.0, 1.0, 1.0]
    assert torch.equal(p_all[1], p0[1])               # u = 0: no movement
    assert bool((p_all[3] != 0).any())                # plain Adam direction
    assert all(0.0 < float(r_all[i]) for i in (0, 4))
    p_wo, r_wo = run([0, 1, 3, 4], 0.0)
    for a, b in zip([0, 1, 3, 4], range(4)):
        assert torch.equal(p_all[a], p_wo[b]), a
        assert float(r_all[a]) == float(r_wo[b]), a
    _, r_wd = run([0, 1, 2, 3, 4], 0.25)
    # u = wd*p exactly (a power of two), so |p|/|u| = 4 within the norms'
    # 36U + 36U + 1U of tests/test_gpu_lars.py
    assert abs(float(r_wd[1]) - 4.0) <= 73 * U * 4.0
    assert r_wd[2:4].tolist() == [1.0, 1.0]


# ----------------------------------------------------------- 3. step counter ---

def test_found_inf_is_a_device_side_no_op():
    ext = _ext()
    sizes = [CH + 1, 7, 0, 3]
    n = len(sizes)
    pv, fp, _ = _pack(_randn(sizes, 71), 1)
    gv, fg, _ = _pack(_randn(sizes, 72), 2)
    mv, fm, _ = _pack(_randn(sizes, 73), 3)
    vv, fv, _ = _pack([t.abs() for t in _randn(sizes, 74)], 0)
    steps, coefs = _counters(n)
    steps[:n] = 5.0
    partials, ratios = _buffers(sizes)
    watched = (fp, fg, fm, fv, steps, coefs, partials, ratios)
    before = [t.clone() for t in watched]
    fi = torch.ones(1, device=DEV)
    for coef in (None, torch.tensor([0.5], device=DEV)):
        ext.fused_lamb(pv, gv, mv, vv, steps, coefs, partials, ratios, 1e-2,
                       0.9, 0.999, 1e-6, 0.05, True, 10.0, fi, coef)
    for got, want in zip(watched, before):
        assert torch.equal(got, want)
    fi.zero_()
    ext.fused_lamb(pv, gv, mv, vv, steps, coefs, partials, ratios, 1e-2, 0.9,
                   0.999, 1e-6, 0.05, True, 10.0, fi, None)
    assert not torch.equal(fp, before[0])
    assert steps.cpu()[:n].tolist() == [6.0] * n
    assert bool((ratios[:n] != GUARD).all())


def make_lamb(ps, half):
    from ddp_tricks_amd.ops.optim import FusedLAMB
    return FusedLAMB([dict(params=ps[:half], weight_decay=0.05),
                      dict(params=ps[half:], adapt=False, weight_decay=0.0)],
                     lr=1e-2, betas=(0.9, 0.99), eps=1e-6)


def test_overflow_step_does_not_advance_the_bias_correction():
    overflow_check(make_lamb)


def test_parameter_without_gradient_keeps_its_step():
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedLAMB
    amp._state.__init__()
    sizes = [7, CH + 1, 5, 3]
    ps, fp, gp = _param_views(_randn(sizes, 61), 1)
    opt = FusedLAMB(ps, lr=1e-2)
    _set_grads(ps, _randn(sizes, 62), 2)
    opt.step()
    r1 = opt.trust_ratios.clone()
    before = [p.detach().clone() for p in ps]
    ps[1].grad = None
    opt.step()
    assert opt._steps.tolist() == [2.0, 1.0, 2.0, 2.0]
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0, 2.0, 2.0]
    assert torch.equal(ps[1].detach(), before[1])
    assert float(opt.trust_ratios[1]) == float(r1[1])
    for i in (0, 2, 3):
        assert not torch.equal(ps[i].detach(), before[i])
    assert _guards_intact(fp, gp)


# ------------------------------------------------------------ 4. composition ---

@pytest.mark.parametrize("lookahead", [False, True])
def test_lazy_clip_equals_in_place_clip(lookahead, monkeypatch):
    lazy_clip_check(make_lamb, lookahead, monkeypatch)


def test_non_adapted_groups_match_fused_adamw():
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedAdamW, FusedLAMB
    amp._state.__init__()
    sa, sb = [CH + 1, 0, 5], [7, 2 * CH + 7, 1, 3]
    a, fa, ga = _param_views(_randn(sa, 41), 1)
    b, fb, gb = _param_views(_randn(sb, 42), 2)
    b2, fb2, _ = _param_views(_randn(sb, 42), 2)
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-7)
    lamb = FusedLAMB([dict(params=a, weight_decay=0.05),
                      dict(params=b, adapt=False, weight_decay=0.02)], **kw)
    adamw = FusedAdamW(b2, weight_decay=0.02, **kw)
    ratios = None
    for step in range(3):
        _set_grads(a, _randn(sa, 50 + step), 3)
        gb_ = _randn(sb, 60 + step)
        _set_grads(b, gb_, 1)
        _set_grads(b2, gb_, 1)
        lamb.step()
        adamw.step()
        assert torch.equal(fb, fb2), step             # params (+ guards)
        for p, q in zip(b, b2):
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(lamb.state[p][key],
                                   adamw.state[q][key]), (step, key)
        r = lamb.trust_ratios
        assert r.device == DEV and r.dtype == torch.float32
        assert r.shape == (len(sa) + len(sb),)
        assert ratios is None or r is ratios          # allocated once
        ratios = r
        got = r.tolist()
        assert got[1] == 1.0 and got[3:] == [1.0] * len(sb)
        assert got[0] > 0.0 and got[2] > 0.0 and got[0] != got[2]
    assert lamb._steps.tolist() == [3.0] * 7
    assert _guards_intact(fa, ga) and _guards_intact(fb, gb)


def test_six_steps_twice_bitwise():
    twice_check(make_lamb)


def test_same_step_helper_sees_ratios():
    """amp_run records the trust ratios of a LAMB run (None for AdamW), so
    the bitwise comparisons above cover them."""
    a = amp_run(make_lamb, [False])
    assert a[0]["ratios"] is not None and a[0]["ratios"].shape == (3,)
    assert same_step(a[0], a[0])
