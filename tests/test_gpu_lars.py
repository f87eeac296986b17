"""GPU tier of FusedLARS: the pair square-sum, per-tensor ratio and step
kernels behind ``ext.fused_lars`` and the optimizer on top of them.

Shapes are the smallest at which the (tensor, 16384-element chunk) mapping
can go wrong: sizes around the chunk edge, a 70-tensor list (three
32-tensor launch groups, so the ratio and partial indices must be global),
views at element offsets that are not 16-byte aligned, and one tensor of
257 chunks + 3 elements (more chunks than the ratio kernel's block has
threads).  Every tensor is carved out of a sentinel-filled flat with one
guard element on each side, so an out-of-range write shows up as a changed
guard value.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

CH = 16384
SIZES = [0, 1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7]
GUARD = -12345.0
U = 2.0 ** -24                  # fp32 unit roundoff
RATIO_RTOL = 74 * U             # see test_random_matches_float64


def _ext():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    assert ext.MT_CHUNK == CH
    return ext


def _cases():
    """name -> (sizes, lead): tensors packed into one flat after `lead`
    elements, one guard element between neighbours."""
    c = {f"n{n}": ([n], 0) for n in SIZES}
    c["all_sizes"] = (SIZES, 0)
    c["seventy_by_5"] = ([5] * 70, 0)
    for off in (1, 2, 3):
        c[f"offset{off}"] = ([CH + 1, 7, 2 * CH + 7], off)
    c["wide"] = ([257 * CH + 3], 0)
    return c


CASES = _cases()
MULTI = ["all_sizes", "seventy_by_5", "offset1", "offset2", "offset3", "wide"]


def _pack(cpu_tensors, lead):
    """Device views of one sentinel flat at arbitrary element offsets (what
    p.grad is inside a DDP bucket).  Returns (views, flat, guard_mask)."""
    total = lead + sum(t.numel() + 1 for t in cpu_tensors) + 1
    flat = torch.full((total,), GUARD, dtype=torch.float32)
    guard = torch.ones(total, dtype=torch.bool)
    spans, pos = [], lead + 1
    for t in cpu_tensors:
        n = t.numel()
        flat[pos:pos + n] = t
        guard[pos:pos + n] = False
        spans.append((pos, n))
        pos += n + 1
    dflat = flat.to(DEV)
    views = [dflat.narrow(0, s, n) for s, n in spans]
    return views, dflat, guard


def _guards_intact(dflat, guard):
    return bool((dflat.cpu()[guard] == GUARD).all())


def _nchunks(sizes):
    return sum((n + CH - 1) // CH for n in sizes)


def _buffers(sizes):
    """Sentinel-filled partials / ratios with three spare floats each."""
    partials = torch.full((2 * _nchunks(sizes) + 3,), GUARD, device=DEV)
    ratios = torch.full((len(sizes) + 3,), GUARD, device=DEV)
    return partials, ratios


def _randn(sizes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in sizes]


# ------------------------------------------------------ 1. exact arithmetic ---

def _spread(n, value, seed):
    """n-element tensor with 4**k entries of +-value (k as large as fits)
    at evenly spread positions that include the first and the last element,
    zeros elsewhere: its 2-norm is |value| * 2**k exactly."""
    t = torch.zeros(n)
    if n == 0:
        return t, 0.0
    count = 1
    while count * 4 <= n:
        count *= 4
    if count == 1:
        pos = torch.tensor([n - 1])
    else:
        pos = (torch.arange(count) * (n - 1)) // (count - 1)
    assert pos.unique().numel() == count
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (count,), generator=g).float() * 2 - 1
    t[pos] = sign * value
    return t, abs(value) * count ** 0.5


@pytest.mark.parametrize("gs", [None, 0.5])
@pytest.mark.parametrize("case", list(CASES))
def test_exact_ratios_and_step(case, gs):
    """p holds +-2**(1 + i%5) and g holds +-1 at 4**k positions each, so
    both norms are powers of two (every partial and total is an integer far
    below 2**24: exact in any order), and with eps = wd = 0 and eta = 2**-8
    the ratio eta*wn/gn is a power of two that must come out exactly.  It
    differs between neighbouring tensors, so a ratio written or read at a
    launch-group-local index shows.  The step must be bitwise
    multi_tensor_scale(g_t, r_t) per tensor followed by fused_sgd."""
    ext = _ext()
    sizes, lead = CASES[case]
    eta, lr, mu = 2.0 ** -8, 0.1, 0.9
    ps, gs_, want = [], [], []
    for i, n in enumerate(sizes):
        p, wn = _spread(n, 2.0 ** (1 + i % 5), 100 + i)
        g, gn = _spread(n, 1.0, 200 + i)
        ps.append(p)
        gs_.append(g)
        if n == 0:
            want.append(1.0)
        else:
            want.append(eta * wn / (gn * (gs or 1.0)))
    b0 = _randn(sizes, 3)
    coef = None if gs is None else torch.tensor([gs], device=DEV)

    pv, fp, gp = _pack(ps, lead)
    gv, fg, gg = _pack(gs_, (lead + 1) % 4)
    bv, fb, gb = _pack(b0, (lead + 2) % 4)
    fg_before = fg.clone()
    partials, ratios = _buffers(sizes)
    ext.fused_lars(pv, gv, bv, partials, ratios, lr, mu, 0.0, 1.0, eta, 0.0,
                   False, None, coef)
    got = ratios.cpu()
    assert got[:len(sizes)].tolist() == want          # exact, global index
    assert bool((got[len(sizes):] == GUARD).all())
    nc = _nchunks(sizes)
    assert bool((partials.cpu()[2 * nc:] == GUARD).all())
    assert torch.equal(fg, fg_before)                 # gradients kept
    assert _guards_intact(fp, gp) and _guards_intact(fb, gb)

    # reference: scale each gradient by its ratio in place, then plain SGD
    p2, fp2, _ = _pack(ps, lead)
    g2, fg2, gg2 = _pack(gs_, (lead + 1) % 4)
    b2, fb2, _ = _pack(b0, (lead + 2) % 4)
    if coef is not None:
        ext.multi_tensor_scale(g2, coef, None)
    for t in range(len(sizes)):
        ext.multi_tensor_scale([g2[t]], ratios[t:t + 1], None)
    ext.fused_sgd(p2, g2, b2, lr, mu, 0.0, 1.0, None, None)
    assert torch.equal(fp, fp2)                       # params (+ guards)
    assert torch.equal(fb, fb2)                       # momentum buffers
    assert _guards_intact(fg2, gg2)
    if sum(sizes):
        assert not torch.equal(fp.cpu()[~gp], torch.cat(ps))     # it stepped


def test_buffers_too_small_is_an_error():
    ext = _ext()
    pv, fp, _ = _pack([torch.ones(CH + 1), torch.ones(3)], 0)    # 3 chunks
    gv, _, _ = _pack([torch.ones(CH + 1), torch.ones(3)], 1)
    before = fp.clone()
    ok_p, ok_r = torch.zeros(6, device=DEV), torch.zeros(2, device=DEV)
    with pytest.raises(RuntimeError, match="partials"):
        ext.fused_lars(pv, gv, [], torch.zeros(5, device=DEV), ok_r, 0.1,
                       0.0, 0.0, 0.0, 0.001, 0.0, False, None, None)
    with pytest.raises(RuntimeError, match="ratios"):
        ext.fused_lars(pv, gv, [], ok_p, torch.zeros(1, device=DEV), 0.1,
                       0.0, 0.0, 0.0, 0.001, 0.0, False, None, None)
    with pytest.raises(RuntimeError):                # grad of another size
        ext.fused_lars(pv, gv[::-1], [], ok_p, ok_r, 0.1, 0.0, 0.0, 0.0,
                       0.001, 0.0, False, None, None)
    assert torch.equal(fp, before)


# ----------------------------------------------------------- 2. random data ---

CONFIGS = [(wd, mu, nest, clip)
           for wd in (0.0, 5e-4)
           for mu, nest in ((0.0, False), (0.9, False), (0.9, True))
           for clip in (False, True)]


def _random_cases():
    out = []
    for case in MULTI:
        cfgs = CONFIGS if case != "wide" else [CONFIGS[5], CONFIGS[6]]
        out += [(case,) + c for c in cfgs]
    return out


@pytest.mark.parametrize("case,wd,mu,nesterov,trust_clip", _random_cases())
def test_random_matches_float64(case, wd, mu, nesterov, trust_clip):
    """Against the formula in float64, one step from identical state (zero
    momentum buffers).

    Ratios.  A chunk's sum of squares is <= 64 sequential fmaf terms per
    thread plus an 8-level tree over positive terms: relative error
    <= 72*U (U = 2**-24, the figure tests/test_gpu_clip.py uses), half of
    it, 36*U, on each norm; the double sum over chunks and the double sqrt
    add nothing at this scale.  The ratio is formed in double from the two
    norms (all terms of the denominator are positive, so its relative error
    is at most the norms') and rounded to fp32 once: 36 + 36 + 1 <= 74*U.

    Step.  With buf = 0 the direction d is linear in the ratio, so the
    ratio's error moves p by at most 74*U * lr*|d_ref| and buf by
    74*U * |buf_ref|.  On top, one rounding per fp32 operation, each
    relative to the absolute-value chain A = |g| + wd*|p|, Dabs =
    (1 + mu or 1) * A * r:  gi = fmaf(wd, p, g) with wd rounded to fp32
    (2), * r (1), buf = fmaf(mu, 0, gi) (0), d = fmaf(mu, buf, gi) with mu
    rounded (2, on top of (1 + mu) times gi's 3), p = fmaf(-lr, d, p) with
    lr rounded (2): |p - p_ref| <= 74*U*lr*|d_ref| + U*(|p| + 8*lr*Dabs),
    |buf - buf_ref| <= 74*U*|buf_ref| + 4*U*A*r."""
    ext = _ext()
    sizes, lead = CASES[case]
    lr, eta, eps = 0.1, 0.02, 1e-8
    p0 = _randn(sizes, 21)
    g0 = _randn(sizes, 22, scale=3.0)
    pv, fp, gp = _pack(p0, lead)
    gv, fg, gg = _pack(g0, (lead + 1) % 4)
    bv, fb, gb = _pack([torch.zeros(n) for n in sizes], (lead + 2) % 4)
    fg_before = fg.clone()
    partials, ratios = _buffers(sizes)
    ext.fused_lars(pv, gv, bv if mu else [], partials, ratios, lr, mu, wd,
                   1.0 if nesterov else 0.0, eta, eps, trust_clip, None, None)
    got_r = ratios.cpu()[:len(sizes)].double()
    assert torch.equal(fg, fg_before)
    assert _guards_intact(fp, gp) and _guards_intact(fb, gb)

    # the gradient half of the partials is bitwise the square-sum kernel's
    nc = _nchunks(sizes)
    ps = torch.zeros(nc, device=DEV)
    ext.multi_tensor_sqsum(gv, ps)
    assert torch.equal(partials[1:2 * nc:2], ps)

    for i, n in enumerate(sizes):
        p, g = p0[i].double(), g0[i].double()
        wn, gn = float(p.norm()), float(g.norm())
        r = 1.0
        if wn > 0 and gn > 0:
            r = eta * wn / (gn + wd * wn + eps)
            if trust_clip:
                r = min(r / lr, 1.0)
        print(f"{case}[{i}] n={n} ratio rel err "
              f"{abs(float(got_r[i]) - r) / r / U:.2f} U")
        assert abs(float(got_r[i]) - r) <= RATIO_RTOL * r, (i, n)
        if n == 0:
            continue
        gi = (g + wd * p) * r
        A = (g.abs() + wd * p.abs()) * r
        if mu != 0:
            buf = gi
            d = gi + mu * buf if nesterov else buf
            Dabs = (1 + mu) * A if nesterov else A
        else:
            buf, d, Dabs = None, gi, A
        p_ref = p - lr * d
        bound = RATIO_RTOL * lr * d.abs() + U * (p.abs() + 8 * lr * Dabs)
        err = (pv[i].cpu().double() - p_ref).abs()
        print(f"    p err/bound max {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (i, n)
        if mu != 0:
            bb = RATIO_RTOL * buf.abs() + 4 * U * A
            berr = (bv[i].cpu().double() - buf).abs()
            assert bool((berr <= bb).all()), (i, n)
    if mu == 0:                                       # buffers never touched
        assert bool((fb.cpu()[~gb] == 0).all())


# ------------------------------------------------------ 3. degenerate tensors ---

def test_degenerate_tensors():
    """Zero gradient and zero parameter tensors get ratio 1 and nothing
    non-finite (eps = 0: no help from the denominator); a zero-size tensor
    between others changes nothing for its neighbours."""
    ext = _ext()
    sizes = [7, CH + 1, 0, 5, 9]
    p0 = _randn(sizes, 31)
    g0 = _randn(sizes, 32)
    g0[1].zero_()
    p0[3].zero_()

    def run(keep):
        pv, fp, gp = _pack([p0[i] for i in keep], 1)
        gv, _, _ = _pack([g0[i] for i in keep], 2)
        bv, fb, gb = _pack([torch.zeros(sizes[i]) for i in keep], 3)
        partials, ratios = _buffers([sizes[i] for i in keep])
        first = None
        for step in range(2):
            ext.fused_lars(pv, gv, bv, partials, ratios, 0.1, 0.9, 5e-4, 1.0,
                           0.02, 0.0, False, None, None)
            if step == 0:
                first = ratios.cpu()[:len(keep)].clone()
        assert _guards_intact(fp, gp) and _guards_intact(fb, gb)
        assert bool(torch.isfinite(fp).all()) and bool(
            torch.isfinite(fb).all())
        return ([v.cpu() for v in pv], [v.cpu() for v in bv], first,
                ratios.cpu()[:len(keep)])

    p_all, b_all, r_first, r_all = run([0, 1, 2, 3, 4])
    assert r_first[1:4].tolist() == [1.0, 1.0, 1.0]
    assert r_all[1:3].tolist() == [1.0, 1.0]          # still a zero gradient
    assert all(0.0 < float(r_all[i]) < 1.0 for i in (0, 3, 4))
    assert bool(torch.isfinite(r_all).all())
    # the all-zero parameter took a plain SGD step on its first step
    assert bool((p_all[3] != 0).any())
    p_wo, b_wo, _, r_wo = run([0, 1, 3, 4])
    for a, b in zip([0, 1, 3, 4], range(4)):
        assert torch.equal(p_all[a], p_wo[b]), a
        assert torch.equal(b_all[a], b_wo[b]), a
        assert float(r_all[a]) == float(r_wo[b]), a


# ------------------------------------------------------ optimizer-level tools ---

def _param_views(cpu_tensors, lead):
    views, flat, guard = _pack(cpu_tensors, lead)
    return [torch.nn.Parameter(v) for v in views], flat, guard


def _set_grads(params, cpu_grads, lead):
    views, flat, guard = _pack(cpu_grads, lead)
    for p, v in zip(params, views):
        p.grad = v
    return flat, guard


def _buf_list(opt, params):
    return [opt.state[p]["momentum_buffer"].clone() for p in params]


# ---------------------------------------------------------- 4. mixed groups ---

def test_mixed_groups_match_fused_sgd():
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedLARS, FusedSGD
    amp._state.__init__()
    sa, sb = [CH + 1, 0, 5], [7, 2 * CH + 7, 1, 3]
    a, fa, ga = _param_views(_randn(sa, 41), 1)
    b, fb, gb = _param_views(_randn(sb, 42), 2)
    b2, fb2, _ = _param_views(_randn(sb, 42), 2)
    lars = FusedLARS([dict(params=a, weight_decay=5e-4),
                      dict(params=b, adapt=False, weight_decay=1e-4)],
                     lr=0.1, momentum=0.9, nesterov=True,
                     trust_coefficient=0.02)
    sgd = FusedSGD(b2, lr=0.1, momentum=0.9, nesterov=True,
                   weight_decay=1e-4)
    ratios = None
    for step in range(3):
        ga_ = _randn(sa, 50 + step)
        gb_ = _randn(sb, 60 + step)
        _set_grads(a, ga_, 3)
        _set_grads(b, gb_, 1)
        _set_grads(b2, gb_, 1)
        lars.step()
        sgd.step()
        assert torch.equal(fb, fb2), step             # params (+ guards)
        for p, q in zip(b, b2):
            assert torch.equal(lars.state[p]["momentum_buffer"],
                               sgd.state[q]["momentum_buffer"]), step
        r = lars.trust_ratios
        assert r.device == DEV and r.dtype == torch.float32
        assert r.shape == (len(sa) + len(sb),)
        assert ratios is None or r is ratios          # allocated once
        ratios = r
        got = r.tolist()
        assert got[1] == 1.0 and got[3:] == [1.0] * len(sb)
        assert 0.0 < got[0] < 1.0 and 0.0 < got[2] < 1.0
    assert _guards_intact(fa, ga) and _guards_intact(fb, gb)


# -------------------------------------------------------------- 5. overflow ---

def test_found_inf_is_a_device_side_no_op():
    ext = _ext()
    sizes = [CH + 1, 7, 0, 3]
    pv, fp, _ = _pack(_randn(sizes, 71), 1)
    gv, fg, _ = _pack(_randn(sizes, 72), 2)
    bv, fb, _ = _pack(_randn(sizes, 73), 3)
    partials, ratios = _buffers(sizes)
    before = [t.clone() for t in (fp, fg, fb, partials, ratios)]
    fi = torch.ones(1, device=DEV)
    for coef in (None, torch.tensor([0.5], device=DEV)):
        ext.fused_lars(pv, gv, bv, partials, ratios, 0.1, 0.9, 5e-4, 1.0,
                       0.02, 1e-8, True, fi, coef)
    for got, want in zip((fp, fg, fb, partials, ratios), before):
        assert torch.equal(got, want)
    fi.zero_()
    ext.fused_lars(pv, gv, bv, partials, ratios, 0.1, 0.9, 5e-4, 1.0, 0.02,
                   1e-8, True, fi, None)
    assert not torch.equal(fp, before[0])
    assert bool((ratios[:len(sizes)] != GUARD).all())


def _amp_run(steps, sizes=(CH + 1, 7, 5), max_grad_norm=None, lookahead=False,
             seed=81):
    """steps: one entry per step, True plants an inf in the loss weights.
    Returns per-step (params, bufs, ratios, lazy)."""
    from ddp_tricks_amd import amp
    from ddp_tricks_amd.ops.optim import FusedLARS
    from ddp_tricks_amd.utils.lookahead import Lookahead
    amp._state.__init__()
    ps, fp, gp = _param_views(_randn(sizes, seed), 1)
    half = len(sizes) - 1
    inner = FusedLARS([dict(params=ps[:half], weight_decay=5e-4),
                       dict(params=ps[half:], adapt=False, weight_decay=0.0)],
                      lr=0.1, momentum=0.9, nesterov=True,
                      trust_coefficient=0.02)
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
        out.append((fp.clone(), _buf_list(inner, ps),
                    inner.trust_ratios.clone(), lazy))
    assert float(amp.state().overflow_count) == sum(steps)
    amp._state.__init__()
    assert _guards_intact(fp, gp)
    return out


def test_overflow_step_through_amp_is_skipped():
    clean = _amp_run([False, False])
    seen = _amp_run([False, True, False])
    p1, b1, r1, _ = seen[0]
    p2, b2, r2, _ = seen[1]                           # the overflow step
    assert torch.equal(p1, p2) and torch.equal(r1, r2)
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))
    assert torch.equal(clean[0][0], p1)
    p3, b3, r3, _ = seen[2]
    assert torch.equal(p3, clean[1][0]) and torch.equal(r3, clean[1][2])
    assert all(torch.equal(x, y) for x, y in zip(b3, clean[1][1]))
    assert not torch.equal(p3, p1)
    assert bool(torch.isfinite(p3).all())


# ------------------------------------------------------ 6. clip composition ---

@pytest.mark.parametrize("lookahead", [False, True])
def test_lazy_clip_equals_in_place_clip(lookahead, monkeypatch):
    monkeypatch.delenv("DDPX_SYNC_AMP", raising=False)
    monkeypatch.delenv("DDPX_CLIP_FUSED", raising=False)
    lazy = _amp_run([False] * 3, max_grad_norm=1.0, lookahead=lookahead)
    monkeypatch.setenv("DDPX_CLIP_FUSED", "0")
    inpl = _amp_run([False] * 3, max_grad_norm=1.0, lookahead=lookahead)
    assert [s[3] for s in lazy] == [True] * 3         # FusedLARS recognised
    assert [s[3] for s in inpl] == [False] * 3
    for step, (a, b) in enumerate(zip(lazy, inpl)):
        assert torch.equal(a[0], b[0]), step          # params (+ guards)
        assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])), step
        assert torch.equal(a[2], b[2]), step          # ratios
    # the clip was active: an unclipped run differs
    free = _amp_run([False] * 3, lookahead=lookahead)
    assert not torch.equal(free[0][2], lazy[0][2])


# ------------------------------------------------------------ 7. determinism ---

def test_six_steps_twice_bitwise():
    def run():
        a = _amp_run([False] * 6, sizes=tuple(SIZES) + (5,) * 70,
                     max_grad_norm=1.0, lookahead=True, seed=91)
        return a
    one, two = run(), run()
    for step, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a[0], b[0]), step
        assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])), step
        assert torch.equal(a[2], b[2]), step
    assert not torch.equal(one[0][0], one[5][0])
    assert bool(torch.isfinite(one[5][0][one[5][0] != GUARD]).all())
