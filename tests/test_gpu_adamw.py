"""GPU tier of FusedAdamW: the step-counter tick and the one-pass step
behind ``ext.fused_adamw`` and the optimizer on top of them.

Shapes and the guarded-flat packing are those of tests/test_gpu_lars.py
(sizes around the 16384-element chunk edge, a 70-tensor list that makes
three launch groups, views at element offsets that are not 16-byte
aligned); every tensor is carved out of a sentinel-filled flat, so an
out-of-range write shows up as a changed guard value.
"""
import copy
import math

import pytest
import torch

from test_gpu_lars import (CASES, CH, GUARD, MULTI, SIZES, U, _ext,
                           _guards_intact, _pack, _param_views, _randn,
                           _set_grads)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

NCOEF = 4
ADAM_CASES = [c for c in CASES if c != "wide"]
ADAM_MULTI = [c for c in MULTI if c != "wide"]


def _counters(n):
    """Sentinel-guarded step and coefficient flats with three spare floats
    each; the steps start at 0."""
    steps = torch.full((n + 3,), GUARD, device=DEV)
    steps[:n] = 0
    coefs = torch.full((NCOEF * n + 3,), GUARD, device=DEV)
    return steps, coefs


def _pow2(sizes, seed, lo=-3, hi=3):
    """+-2**k in every element, k uniform in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        k = torch.randint(lo, hi + 1, (n,), generator=g).float()
        s = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
        out.append(s * torch.exp2(k))
    return out


def coef_ref(lr, b1, b2, step):
    """The tick's four coefficients in double."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return [lr / bc1, math.sqrt(bc2), bc1, bc2]


# ------------------------------------------------------ 1. exact first step ---

@pytest.mark.parametrize("gs", [None, 0.5])
@pytest.mark.parametrize("case", ADAM_CASES)
def test_exact_first_step(case, gs):
    """betas = (0.5, 0.75), eps = 0, m = v = 0, every g = +-2**k, lr = 2**-6
    and lr*wd = 2**-9.  Then every intermediate is a power of two or exact:
    m = g/2, v = g*g/4, bc1 = 1/2, bc2 = 1/4, lr/bc1 = 2**-5, sqrt(bc2) =
    1/2, sqrt(v)/sqrt(bc2) = |g|, m/|g| = sign(g)/2, and the step is
    p*(1 - lr*wd) - lr*sign(g) with one rounding in the product and one in
    the difference, which is what the fp32 expression below does."""
    ext = _ext()
    sizes, lead = CASES[case]
    lr, wd = 2.0 ** -6, 2.0 ** -3
    p0 = _randn(sizes, 11)
    g0 = _pow2(sizes, 12)
    zeros = [torch.zeros(n) for n in sizes]
    coef = None if gs is None else torch.tensor([gs], device=DEV)
    pv, fp, gp = _pack(p0, lead)
    gv, fg, gg = _pack(g0, (lead + 1) % 4)
    mv, fm, gm = _pack(zeros, (lead + 2) % 4)
    vv, fv, gv_ = _pack(zeros, (lead + 3) % 4)
    fg_before = fg.clone()
    steps, coefs = _counters(len(sizes))
    ext.fused_adamw(pv, gv, mv, vv, steps, coefs, lr, 0.5, 0.75, 0.0, wd,
                    True, None, coef)
    n = len(sizes)
    assert steps.cpu()[:n].tolist() == [1.0] * n
    assert bool((steps.cpu()[n:] == GUARD).all())
    want_c = torch.tensor([2 * lr, 0.5, 0.5, 0.25] * n)
    assert torch.equal(coefs.cpu()[:NCOEF * n], want_c)
    assert bool((coefs.cpu()[NCOEF * n:] == GUARD).all())
    assert torch.equal(fg, fg_before)                 # gradients kept
    for i in range(n):
        ge = g0[i] * (gs or 1.0)
        assert torch.equal(mv[i].cpu(), 0.5 * ge), i
        assert torch.equal(vv[i].cpu(), 0.25 * ge * ge), i
        want_p = p0[i] * (1.0 - lr * wd) - lr * torch.sign(g0[i])
        assert torch.equal(pv[i].cpu(), want_p), i
    assert _guards_intact(fp, gp) and _guards_intact(fm, gm)
    assert _guards_intact(fv, gv_) and _guards_intact(fg, gg)


def test_operand_checks():
    ext = _ext()
    t = [torch.ones(CH + 1), torch.ones(3)]
    pv, fp, _ = _pack(t, 0)
    gv, _, _ = _pack(t, 1)
    mv, _, _ = _pack(t, 2)
    vv, _, _ = _pack(t, 3)
    before = fp.clone()
    steps, coefs = torch.zeros(2, device=DEV), torch.zeros(8, device=DEV)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, True, None, None)
    with pytest.raises(RuntimeError, match="steps"):
        ext.fused_adamw(pv, gv, mv, vv, steps[:1], coefs, *args)
    with pytest.raises(RuntimeError, match="coefs"):
        ext.fused_adamw(pv, gv, mv, vv, steps, coefs[:7], *args)
    with pytest.raises(RuntimeError):                 # grad of another size
        ext.fused_adamw(pv, gv[::-1], mv, vv, steps, coefs, *args)
    with pytest.raises(RuntimeError, match="exp_avg"):
        ext.fused_adamw(pv, gv, mv[::-1], vv, steps, coefs, *args)
    with pytest.raises(RuntimeError):                 # cpu operand
        ext.fused_adamw(pv, gv, mv, vv, steps.cpu(), coefs, *args)
    assert torch.equal(fp, before)
    assert steps.tolist() == [0.0, 0.0]


# ----------------------------------------------------------- 2. random data ---

def adam_moments_ref(g, m, v, b1, b2):
    """float64 moments and their absolute-value chain M >= |m_new|."""
    m_new = b1 * m + (1 - b1) * g
    M = b1 * m.abs() + (1 - b1) * g.abs()
    v_new = b2 * v + (1 - b2) * g * g
    return m_new, v_new, M


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("case", ADAM_MULTI)
def test_random_matches_float64(case, wd):
    """Three steps against the documented formula in float64, each step's
    reference started from the state the kernel left (so the bound is the
    error of one pass).  The second step's gradients hold a zero tensor and
    scattered zeros.  U = 2**-24; every constant is a double rounded to
    fp32 once (relative error U); first-order terms, the count rounded up
    by one where it closes the second-order remainder.

    m = fma(b1, m, (1-b1)*g): the product carries its constant's and its
    own rounding (2U*(1-b1)|g|), b1's rounding U*b1|m|, the fma's U*M with
    M = b1|m| + (1-b1)|g|:                       |m - m_ref| <= 3U*M
    v = fma(b2, v, ((1-b2)*g)*g): 3U on the product, U on b2*v, U on the
    sum, all terms non-negative:                 v relative  <= 4U
    s = sqrt(v): 2U + U = 3U;  q = s / sqrt(bc2): + U (constant) + U = 5U;
    d = q + eps, positive terms, eps relative U: d relative  <= 6U
    r = m / d: (3U*M + 6U*|m_ref|)/d + U*|r|  <= 10U * M/d
    p' = p * (1 - lr*wd): 2U*|p|
    p = fma(-c0, r, p'), c0 = lr/bc1 relative U, with R = c0*M/d:
        U*R + 10U*R + 2U*|p| + U*(|p| + R) = U*(3|p| + 12R)
    asserted as U*(4|p| + 13R), and 4U*M / 5U*v for the moments."""
    ext = _ext()
    sizes, lead = CASES[case]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    n = len(sizes)
    pv, fp, gp = _pack(_randn(sizes, 21), lead)
    mv, fm, gm = _pack([torch.zeros(k) for k in sizes], (lead + 2) % 4)
    vv, fv, gvv = _pack([torch.zeros(k) for k in sizes], (lead + 3) % 4)
    steps, coefs = _counters(n)
    worst = 0.0
    for step in (1, 2, 3):
        g0 = _randn(sizes, 30 + step, scale=3.0)
        if step == 2:
            g0[1 % n].zero_()
            for g in g0:
                g[::3] = 0
        gv, fg, gg = _pack(g0, (lead + 1) % 4)
        before = [[t.cpu().double() for t in lst] for lst in (pv, mv, vv)]
        ext.fused_adamw(pv, gv, mv, vv, steps, coefs, lr, b1, b2, eps, wd,
                        True, None, None)
        assert steps.cpu()[:n].tolist() == [float(step)] * n
        c_ref = torch.tensor(coef_ref(lr, b1, b2, step) * n,
                             dtype=torch.float64)
        c_err = (coefs.cpu()[:NCOEF * n].double() - c_ref).abs()
        assert bool((c_err <= 1.001 * U * c_ref).all())   # one rounding
        c0, c1 = coef_ref(lr, b1, b2, step)[:2]
        for i in range(n):
            p, m, v = (before[k][i] for k in range(3))
            g = g0[i].double()
            m_ref, v_ref, M = adam_moments_ref(g, m, v, b1, b2)
            d = v_ref.sqrt() / c1 + eps
            R = c0 * M / d
            p_ref = p * (1 - lr * wd) - c0 * m_ref / d
            assert bool(((mv[i].cpu().double() - m_ref).abs()
                         <= 4 * U * M).all()), (step, i)
            assert bool(((vv[i].cpu().double() - v_ref).abs()
                         <= 5 * U * v_ref).all()), (step, i)
            err = (pv[i].cpu().double() - p_ref).abs()
            bound = U * (4 * p.abs() + 13 * R)
            if err.numel():
                worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (step, i)
        assert _guards_intact(fg, gg)
    print(f"{case} wd={wd}: p err/bound max {worst:.3f}")
    assert _guards_intact(fp, gp) and _guards_intact(fm, gm)
    assert _guards_intact(fv, gvv)
    assert bool((steps.cpu()[n:] == GUARD).all())
    assert bool((coefs.cpu()[NCOEF * n:] == GUARD).all())


def _dyadic(sizes, seed):
    """multiples of 2**-8 in [-16, 16]"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-4096, 4097, (k,), generator=g).float() / 256
            for k in sizes]


def test_coupled_decay_is_the_gradient_plus_wd_p():
    """decoupled=False adds wd*p to g before the moments and leaves p
    undecayed.  With wd = 2**-3 and p, g multiples of 2**-8 below 16 the
    sum g + wd*p has 16 significant bits and is exact in fp32, so the step
    must be bitwise the wd = 0 step on that gradient."""
    ext = _ext()
    sizes, lead = CASES["all_sizes"]
    wd = 2.0 ** -3
    p0, g0 = _dyadic(sizes, 41), _dyadic(sizes, 42)
    m0 = _randn(sizes, 43)
    v0 = [t.abs() for t in _randn(sizes, 44)]
    g2 = [g + wd * p for g, p in zip(g0, p0)]
    out = []
    for grads, w, dec in ((g0, wd, False), (g2, 0.0, False), (g2, 0.0, True)):
        pv, fp, gp = _pack(p0, lead)
        gv, _, _ = _pack(grads, 1)
        mv, fm, _ = _pack(m0, 2)
        vv, fv, _ = _pack(v0, 3)
        steps, coefs = _counters(len(sizes))
        ext.fused_adamw(pv, gv, mv, vv, steps, coefs, 1e-3, 0.9, 0.999,
                        1e-8, w, dec, None, None)
        assert _guards_intact(fp, gp)
        out.append((fp, fm, fv))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    for a, b in zip(out[1], out[2]):                  # wd = 0: same kernel path
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0].cpu()[~gp], torch.cat(p0))


@pytest.mark.parametrize("case", ["all_sizes", "seventy_by_5", "offset3"])
def test_grad_scale_equals_scale_then_step(case):
    """GS reads g as __fmul_rn(g, gs): bitwise multi_tensor_scale in place
    followed by the plain kernel, and the gradients stay unwritten."""
    ext = _ext()
    sizes, lead = CASES[case]
    coef = torch.tensor([0.37], device=DEV)
    out = []
    for lazy in (True, False):
        pv, fp, gp = _pack(_randn(sizes, 51), lead)
        gv, fg, _ = _pack(_randn(sizes, 52, scale=3.0), (lead + 1) % 4)
        mv, fm, _ = _pack(_randn(sizes, 53), (lead + 2) % 4)
        vv, fv, _ = _pack([t.abs() for t in _randn(sizes, 54)],
                          (lead + 3) % 4)
        steps, coefs = _counters(len(sizes))
        fg_before = fg.clone()
        if not lazy:
            ext.multi_tensor_scale(gv, coef, None)
        ext.fused_adamw(pv, gv, mv, vv, steps, coefs, 1e-2, 0.9, 0.999,
                        1e-8, 0.05, True, None, coef if lazy else None)
        if lazy:
            assert torch.equal(fg, fg_before)
        assert _guards_intact(fp, gp)
        out.append((fp, fm, fv, steps, coefs))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ----------------------------------------------------------- 3. step counter ---

def test_found_inf_is_a_device_side_no_op():
    ext = _ext()
    sizes = [CH + 1, 7, 0, 3]
    pv, fp, _ = _pack(_randn(sizes, 71), 1)
    gv, fg, _ = _pack(_randn(sizes, 72), 2)
    mv, fm, _ = _pack(_randn(sizes, 73), 3)
    vv, fv, _ = _pack([t.abs() for t in _randn(sizes, 74)], 0)
    steps, coefs = _counters(len(sizes))
    steps[:len(sizes)] = 5.0
    watched = (fp, fg, fm, fv, steps, coefs)
    before = [t.clone() for t in watched]
    fi = torch.ones(1, device=DEV)
    for coef in (None, torch.tensor([0.5], device=DEV)):
        for dec in (True, False):
            ext.fused_adamw(pv, gv, mv, vv, steps, coefs, 1e-2, 0.9, 0.999,
                            1e-8, 0.05, dec, fi, coef)
    for got, want in zip(watched, before):
        assert torch.equal(got, want)
    fi.zero_()
    ext.fused_adamw(pv, gv, mv, vv, steps, coefs, 1e-2, 0.9, 0.999, 1e-8,
                    0.05, True, fi, None)
    assert not torch.equal(fp, before[0])
    assert steps.cpu()[:len(sizes)].tolist() == [6.0] * len(sizes)
    assert bool((coefs[:NCOEF * len(sizes)] != GUARD).all())


def make_adamw(ps, half):
    from ddp_tricks_amd.ops.optim import FusedAdamW
    return FusedAdamW([dict(params=ps[:half], weight_decay=0.05),
                       dict(params=ps[half:], weight_decay=0.0)],
                      lr=1e-2, betas=(0.9, 0.99), eps=1e-8)


def amp_run(make, steps, sizes=(CH + 1, 7, 5), max_grad_norm=None,
            lookahead=False, seed=81):
    """steps: one entry per step, True plants an inf in the loss weights.
    Returns per-step dicts of clones: p (the flat with its guards), m, v
    (lists), steps, ratios (None for AdamW) and whether the clip was
    lazy."""
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.utils.lookahead import Lookahead
    amp._state.__init__()
    ps, fp, gp = _param_views(_randn(sizes, seed), 1)
    inner = make(ps, len(sizes) - 1)
    opt = Lookahead(inner, k=2, alpha=0.5) if lookahead else inner
    _, opt = amp.initialize(None, opt, opt_level="O1",
                            max_grad_norm=max_grad_norm)
    out, clean = [], 0
    for bad in steps:
        # the k-th clean step sees the same weights whatever came between
        ws = _randn(sizes, seed + 100 + clean)
        if bad:
            ws[0][CH - 3] = float("inf")
        else:
            clean += 1
        opt.zero_grad()
        loss = sum((p * w.to(DEV)).sum() + 0.5 * (p * p).sum()
                   for p, w in zip(ps, ws))
        with amp.scale_loss(loss, opt) as sl:
            sl.backward()
        lazy = amp.pending_grad_scale() is not None
        opt.step()
        ratios = getattr(inner, "trust_ratios", None)
        out.append(dict(
            p=fp.clone(),
            m=[inner.state[p]["exp_avg"].clone() for p in ps],
            v=[inner.state[p]["exp_avg_sq"].clone() for p in ps],
            steps=inner._steps.clone(),
            step_views=[float(inner.state[p]["step"]) for p in ps],
            ratios=None if ratios is None else ratios.clone(), lazy=lazy))
    assert float(amp.state().overflow_count) == sum(steps)
    amp._state.__init__()
    assert _guards_intact(fp, gp)
    return out


def same_step(a, b):
    return (torch.equal(a["p"], b["p"]) and torch.equal(a["steps"], b["steps"])
            and all(torch.equal(x, y) for x, y in zip(a["m"], b["m"]))
            and all(torch.equal(x, y) for x, y in zip(a["v"], b["v"]))
            and (a["ratios"] is None or torch.equal(a["ratios"], b["ratios"])))


def overflow_check(make):
    """Three steps with an overflow on the second equal two clean steps,
    bit for bit: the skipped step advanced neither the state nor the bias
    correction."""
    clean = amp_run(make, [False, False])
    seen = amp_run(make, [False, True, False])
    assert same_step(seen[0], clean[0])
    assert same_step(seen[1], seen[0])                # the overflow step
    assert seen[1]["step_views"] == [1.0] * 3
    assert same_step(seen[2], clean[1])
    assert seen[2]["steps"].tolist() == [2.0] * 3
    assert seen[2]["step_views"] == [2.0] * 3
    assert not torch.equal(seen[2]["p"], seen[0]["p"])
    assert bool(torch.isfinite(seen[2]["p"]).all())


def test_overflow_step_does_not_advance_the_bias_correction():
    overflow_check(make_adamw)


def test_parameter_without_gradient_keeps_its_step():
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedAdamW
    amp._state.__init__()
    sizes = [7, CH + 1, 5, 3]
    ps, fp, gp = _param_views(_randn(sizes, 61), 1)
    opt = FusedAdamW(ps, lr=1e-2)
    _set_grads(ps, _randn(sizes, 62), 2)
    opt.step()
    before = fp.clone()
    ps[1].grad = None
    ps[2].grad = None
    opt.step()
    assert opt._steps.tolist() == [2.0, 1.0, 1.0, 2.0]
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0, 1.0, 2.0]
    for i in (1, 2):
        assert torch.equal(ps[i].detach(), before.narrow(
            0, ps[i].storage_offset(), sizes[i]))
    for i in (0, 3):
        assert not torch.equal(ps[i].detach(), before.narrow(
            0, ps[i].storage_offset(), sizes[i]))
    assert _guards_intact(fp, gp)
    # a parameter that never had a gradient has no state and step 0
    qs, _, _ = _param_views(_randn([3, 4], 63), 0)
    opt2 = FusedAdamW(qs, lr=1e-2)
    qs[1].grad = torch.ones(4, device=DEV)
    opt2.step()
    assert opt2._steps.tolist() == [0.0, 1.0]
    assert qs[0] not in opt2.state
    # state_dict: torch's names, step a private 0-dim fp32 device copy
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    st = sd["state"][1]["step"]
    assert st.dim() == 0 and st.dtype == torch.float32 and st.device == DEV
    assert float(st) == 1.0
    assert st.untyped_storage().nbytes() == 4         # not a view of the flat
    opt3 = FusedAdamW(ps, lr=1e-2)
    opt3.load_state_dict(copy.deepcopy(sd))
    assert opt3._steps.tolist() == [2.0, 1.0, 1.0, 2.0]
    assert opt3._steps.device == DEV
    opt3.step()
    assert opt3._steps.tolist() == [3.0, 1.0, 1.0, 3.0]
    assert float(opt3.state[ps[0]]["step"]) == 3.0


# ------------------------------------------------------------ 4. composition ---

def lazy_clip_check(make, lookahead, monkeypatch):
    monkeypatch.delenv("DDPX_SYNC_AMP", raising=False)
    monkeypatch.delenv("DDPX_CLIP_FUSED", raising=False)
    lazy = amp_run(make, [False] * 3, max_grad_norm=1.0, lookahead=lookahead)
    monkeypatch.setenv("DDPX_CLIP_FUSED", "0")
    inpl = amp_run(make, [False] * 3, max_grad_norm=1.0, lookahead=lookahead)
    assert [s["lazy"] for s in lazy] == [True] * 3    # the class is recognised
    assert [s["lazy"] for s in inpl] == [False] * 3
    for step, (a, b) in enumerate(zip(lazy, inpl)):
        assert same_step(a, b), step
    # the clip was active: an unclipped run differs
    monkeypatch.delenv("DDPX_CLIP_FUSED")
    free = amp_run(make, [False] * 3, lookahead=lookahead)
    assert not torch.equal(free[0]["m"][0], lazy[0]["m"][0])


@pytest.mark.parametrize("lookahead", [False, True])
def test_lazy_clip_equals_in_place_clip(lookahead, monkeypatch):
    lazy_clip_check(make_adamw, lookahead, monkeypatch)


def twice_check(make):
    def run():
        return amp_run(make, [False] * 6, sizes=tuple(SIZES) + (5,) * 70,
                       max_grad_norm=1.0, lookahead=True, seed=91)
    one, two = run(), run()
    for step, (a, b) in enumerate(zip(one, two)):
        assert same_step(a, b), step
    assert not torch.equal(one[0]["p"], one[5]["p"])
    last = one[5]["p"]
    assert bool(torch.isfinite(last[last != GUARD]).all())
    assert set(one[5]["steps"].tolist()) == {6.0}


def test_six_steps_twice_bitwise():
    twice_check(make_adamw)
