"""BatchNorm, pooling and cross-entropy kernels against CPU float64
references: exact where the arithmetic allows it, element-wise derived
bands everywhere else.  All tests @pytest.mark.gpu.

Notation.  u = 2^-24 is the fp32 unit roundoff: every fp32 +, *, /, fmaf
rounds once with relative error <= u (hipcc's default division is correctly
rounded; a contracted a*b+c rounds once instead of twice, so counting the
uncontracted roundings covers both).  A library function with an error of R
ulp has relative error <= 2*R*u (one ulp is at most 2^-23 of the value).
bf16(v) is round-to-nearest-even to bf16; it is monotone, which is what the
band check uses:

    the kernel computes an fp32 value f with |f - ref| <= e and stores
    bf16(f), so  bf16(ref - e) <= y <= bf16(ref + e)  must hold element by
    element (rounding the float64 bounds through fp32 first keeps the
    inequality, both roundings are monotone and f is an fp32 number).

Every e below is multiplied by (1 + 2^-10) to absorb the second-order
terms (products of two relative errors of a few hundred u at most).

Host geometry, mirrored from bn.hip by ``_geom`` (C % 8 == 0, C/8 <= 256):
    cpg = C/8, block = (256 // cpg) * cpg, nw = block // cpg walkers
    partial sums:  S = clamp(M // (4*nw), 1, 1024) blocks, walker (s, w)
                   starts at row s*nw + w and steps S*nw rows; backward
                   partial is unrolled 2-deep with a one-row tail loop
    dx:            dxblocks = clamp(M // (2*nw), 1, 2048), row stride
                   dxblocks*nw, 2-deep unroll plus tail
    apply:         tv = M*C/8 vectors, blocks = min(4096, ceil(tv/256)),
                   stride = blocks*256; the 2-deep main loop runs only for
                   threads with i + stride < tv
    pool2 bwd:     S = clamp(Mp // (4*nw), 1, 1024),
                   dxblocks = clamp(Mp // nw, 1, 2048) over Mp = M/4 pooled
                   rows, plain strided loops

1. BN backward, exact (bn_bwd, bn_bwd_pool2).  The kernels take save_mean
   and save_invstd as inputs, so the test feeds dyadic ones: mean in
   {-1, 0, 1}, invstd in {0.5, 1, 2}, gamma in {+-0.5, +-1, +-2}, x integers
   in {-4..4}, dy in {-2..2}.  xhat = (x - mean) * invstd is then an exact
   multiple of 0.5 with |xhat| <= 10 and every term of sum(dy_eff) and
   sum(dy_eff * xhat) is a multiple of 0.5.  Multiples of 0.5 below 2^23
   are fp32 numbers, so while sum|terms| < 2^23 (asserted on the reference)
   the sums are exact in any order: dgamma, dbeta ``torch.equal``.  dresid
   is the masked dy, exact.  With eval_stats the host zeroes coef_b and
   coef_c, dx = (gamma*invstd) * dy_eff, a product with a power of two:
   exact for any M.  Otherwise dx = ca * (g - cb - xhat*cc), cb = dbeta/M,
   cc = dgamma/M.  For M a power of two <= 4096 the divisions are exact,
   |dgamma| < 2^18 halves gives cc at most 18 significant bits, xhat 5, so
   the product (23 bits), both differences (multiples of 2^-14 below 2^8)
   and the scaling by ca (a power of two) are all fp32 numbers, with or
   without contraction.  The test asserts that on the float64 reference
   (every intermediate survives a round trip through fp32) and compares dx
   with the reference rounded once to bf16.  For other M:
       cb, cc        one rounding each (the division)
       xhat * cc     one more, g - cb one, the second difference one
   so no term passes more than three roundings and
       e = 3u * |ca| * (|g| + |cb| + |xhat*cc|).

2. BN forward statistics (k_bn_partial, k_bn_combine).  Sums: a term passes
   at most L + T additions, L = ceil(M / (S*nw)) in its walker, T = nw (LDS
   sum over walkers) + ceil(S/64) (lane sweep of the slab) + 6 (shuffle
   tree); gamma_s = (L + T)*u as in test_gpu_wgrad_bias.py (x*x of a bf16
   value is exact in fp32, the fmaf rounds once).  On integer data with
   sum|x| and sum x^2 below 2^24 the sums are exact, gamma_s = 0.
       mean = fl(sum/M):    e_mean = gamma_s*sum|x|/M + u*|mean|
       msq  = fl(sq/M):     e_msq  = gamma_s*sum(x^2)/M + u*msq
     (the u terms vanish when the sums are exact and M is a power of two)
       var = fl(msq - fl(mean*mean)):
                e_var = e_msq + 2|mean|*e_mean + e_mean^2
                        + 3u*(msq + mean^2)
     (u*mean^2 for the product, u*(msq + mean^2) for the difference, one u
     spare; fmaxf(var, 0) only moves var towards the non-negative truth)
       a = fl(var + eps) lies in [(var+eps-e_var)(1-u), (var+eps+e_var)(1+u)]
       invstd = rsqrtf(a): between hi_a^-1/2 * (1 - 2*R_rsqrt*u) and
                lo_a^-1/2 * (1 + 2*R_rsqrt*u) -- an interval, not a
                linearisation, so it stays rigorous when var nearly cancels.
     In the issue's terms this is the relative bound (c + 2R)*u with
     c = ((msq + mean^2)*3 / (var + eps) + 1) / 2 per channel.
       unbiased = var*M/(M-1): two more roundings (M > 1 only; at M = 1 the
                kernel keeps the biased value)
       running = fl(fl(a1*old) + fl(mom*new)), a1 = fl(1 - fl(0.1)) taken in
                fp32 like the kernel: each term passes two roundings,
                e = mom*e_new + 2u*(|a1*old| + mom*|new|).
   The random tier runs bf16 randn data scaled to mean/std = 0, 4 and 32;
   the third measures the E[x^2] - E[x]^2 cancellation the kernel accepts.

3. BN apply (k_bn_apply_v8 behind bn_fwd_train / _eval / _eval_mask).
       sc = fl(gamma * invstd):  e_sc = |gamma| * (invstd interval of 2.,
                                 widened by u for the product)
       sh = fl(beta - fl(mean*sc)):  e_sh = |mean|*e_sc + e_mean*(|sc|+e_sc)
                                 + 2u*(|beta| + |mean*sc|)
       y  = fmaf(x, sc, sh) (+ resid): two more roundings
       e  = |x|*e_sc + e_sh + 2u*(|x*sc| + |mean*sc| + |beta| + |resid|)
   which is the k*u*(|x*sc| + |mean*sc| + |beta| + |resid|) of the issue
   with k = e_sc/(u*|sc|) + 4 per channel (k = 2*R_rsqrt + 6 in eval mode,
   where invstd = rsqrtf(fl(running_var + eps)) has no statistics error).
   Mask bit = (ref > 0) and (y > 0) == bit wherever |ref| > e; the share of
   elements left out is asserted <= 0.1 % on the reference alone (measured:
   at most 1.6e-7, see below).

4. Pooling.  Max-pool is selection: y, the window-local argmax byte and dx
   (sums of at most 9 integers of magnitude <= 2) are exact.  torch's CPU
   max_pool2d scans a window row-major and keeps the first maximum, the
   kernel's strict '>' rule.  Global average pool: integer data, H*W a
   power of two: sum exact, 1/HW exact: ``torch.equal``.  H*W = 49:
   inv = fl(1/49) and one product, e = 2u*|ref|.

5. Cross-entropy.  Thread-per-row: s = sum_c expf(fl(x_c - mx)); the
   argument rounds once (abs. error u*|x_c - mx|, the same relative error
   of the exponential), expf adds 2*R_exp*u, the term then passes at most C
   additions.  Wave-per-row (online softmax): a lane holds E = 8*ceil(C/512)
   elements; a term is rescaled by expf(m_old - m_new) each time the lane
   maximum moves (at most E-1 times) and once per shuffle level (6); the
   rescale arguments telescope, so the argument roundings of a term add up
   to u*(mx - x_c) again.  Per term, relative:
       u * ((mx - x_c) + 2*R_exp*K_exp + K_rnd)
       thread-per-row:  K_exp = 1,      K_rnd = C
       wave-per-row:    K_exp = E + 6,  K_rnd = E + (E-1) + 12
   e_s = sum of that over the row, plus 1e-30 for terms that underflow.
       lse = fl(logf(s) + mx):  e_lse = e_s/s + 2*R_log*u*|log s| + u*|lse|
       rowloss = fl(lse - x_t): e_row = e_lse + u*|rowloss|
       loss = mean: ceil(B/256) serial adds + 8 tree levels + the division:
              e_loss = mean(e_row) + (ceil(B/256) + 9)*u*mean|rowloss|
       dlogits = fl(fl(p - [c == t]) * g), p = expf(fl(x - lse)),
              g = fl(dloss/B):
              e = g*(p*(e_lse + u*|x - lse| + 2*R_exp*u) + 3u*|p - [c == t]|)
     The issue writes the last term as "+ u"; three roundings act on it
     (the difference, g, the product), so 3u*|p - [c == t]| is the derived
     figure, smaller than u wherever |p - [c == t]| < 1/3.  The test takes
     the smaller of the two element by element, never more than the issue
     allows; above 1/3 that relies on the three roundings not all falling
     the same way, which holds on every case here (0 elements outside).
     2^-125 is added for probabilities and products in the subnormal range,
     where a result may be flushed.
   sum_c dlogits is zero in exact arithmetic; the stored bf16 values add a
   rounding each (bf16 unit roundoff 2^-8):
   |sum_c y_c| <= sum_c (e_c + 2^-8*(|ref_c| + e_c)).

Measured constants (MI355X, ROCm 7.0.2; no accuracy table ships with the
toolkit, so ``test_math_function_ulp_errors`` measures each function through
an entry point that exposes its fp32 result unrounded, and holds it to R =
twice the measured maximum, rounded up to a whole ulp):
    rsqrtf: 0.747 ulp over 2048 arguments in [1e-5, 1e3]     -> R_rsqrt = 2
    expf:   0.808 ulp over 65536 arguments in [-100, 10]     -> R_exp = 2
    logf:   2.173 ulp over the integers s = 1..1000          -> R_log = 5
Integer tier: save_invstd is within 1.36 u of float64 (bound 4.5 - 11 u,
153 u at M = 2 where var nearly cancels against mean^2).
Random tier, worst channel, |var_kernel - var| / var measured (bound):
    mean/std  (5, 24)          (2,64,13,13)     (45, 1032)       (6151, 2048)
       0   2.5e-7 (4.6e-5)  2.3e-7 (3.5e-6)  2.5e-7 (2.8e-6)  2.4e-7 (2.2e-6)
       4   5.6e-6 (2.0e-3)  3.5e-6 (1.8e-4)  4.1e-6 (9.7e-5)  4.6e-6 (1.0e-4)
      32   1.0e-3 (1.9e-1)  1.9e-4 (1.1e-2)  2.6e-4 (6.3e-3)  2.1e-4 (6.4e-3)
The E[x^2] - E[x]^2 form loses about (mean/std)^2 * u of the variance.
Left-out share of the mask checks: 0 on 86 of 87 cases, 1.6e-7 on one.
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
R_RSQRT = 2
R_EXP = 2
R_LOG = 5
TINY = 2.0 ** -125      # results in or below the fp32 subnormal range
MOM = 0.1
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
MOM32 = float(torch.tensor(MOM, dtype=torch.float32))
ONE_MINUS_MOM32 = float(torch.tensor(1.0, dtype=torch.float32)
                        - torch.tensor(MOM, dtype=torch.float32))


# ---------------------------------------------------------------- helpers ---

def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _gen(*key):
    return torch.Generator().manual_seed(_seed(*key))


def _ints(shape, lo, hi, *key):
    return torch.randint(lo, hi + 1, tuple(shape),
                         generator=_gen(shape, lo, hi, *key)).double()


def _choice(values, n, *key):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), (n,), generator=_gen(n, *key))]


def _randn(shape, *key):
    return torch.randn(tuple(shape), generator=_gen(shape, *key))


def _randn_bf16(shape, *key):
    return _randn(shape, *key).to(BF).double()


def _cdiv(a, b):
    return -(-a // b)


def _pow2(n):
    return n & (n - 1) == 0


def _mc(shape):
    if len(shape) == 4:
        return shape[0] * shape[2] * shape[3], shape[1]
    return shape


def _sid(shape):
    return "x".join(map(str, shape))


def _dev(rows, shape, dtype=BF):
    """[M, C] CPU rows -> device tensor of ``shape``: 2-D as is, 4-D as an
    NCHW view of channels_last memory."""
    t = rows.to(dtype)
    if len(shape) == 4:
        N, C, H, W = shape
        t = t.view(N, H, W, C).permute(0, 3, 1, 2)
    t = t.to(DEV)
    if len(shape) == 4:
        assert t.is_contiguous(memory_format=torch.channels_last)
    return t


def _rows(t):
    """device output -> [M, C] float64 CPU rows"""
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.cpu().double()


def _f32(v):
    return v.float().to(DEV)


def _fp32_exact(t):
    return torch.equal(t.float().double(), t)


def _bf(t64):
    """float64 -> fp32 -> bf16 -> float64 (both roundings monotone)"""
    return t64.float().to(BF).double()


def _geom(M, C):
    cpg = C // 8
    assert C % 8 == 0 and cpg <= 256
    block = (256 // cpg) * cpg
    nw = block // cpg
    S = max(1, min(1024, M // (4 * nw)))
    dxb = max(1, min(2048, M // (2 * nw)))
    tv = M * cpg
    blocks = min(4096, _cdiv(tv, 256))
    return dict(cpg=cpg, block=block, nw=nw, S=S, dxblocks=dxb, tv=tv,
                stride=blocks * 256,
                L=_cdiv(M, S * nw), T=nw + _cdiv(S, 64) + 6)


def _trip_counts(n, step):
    """iteration counts of the strided loops ``for (i = i0; i < n; i +=
    step)`` over all starts i0 < min(step, n): a count k runs k // 2
    unrolled trips and k % 2 tail iterations"""
    return {_cdiv(n - i0, step) for i0 in (0, min(step, n) - 1)}


def _pack_mask(bits):
    M, C = bits.shape
    w = (1 << torch.arange(8, dtype=torch.int32))
    return (bits.view(M, C // 8, 8).to(torch.int32) * w).sum(-1) \
        .to(torch.uint8)


def _unpack_mask(mask, C):
    m = mask.cpu().to(torch.int32)
    bits = (m.unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1
    return bits.reshape(m.shape[0], C).bool()


def _assert_band(got, ref, e, what, relu=False):
    lo, hi = ref - e, ref + e
    if relu:
        lo, hi = lo.clamp_min(0), hi.clamp_min(0)
        ref = ref.clamp_min(0)
    lo, hi = _bf(lo), _bf(hi)
    bad = ~((got >= lo) & (got <= hi))      # a NaN is outside
    print(f"{what}: max |got - ref| {(got - ref).abs().max().item():.3e}, "
          f"max e {e.max().item():.3e}, outside {int(bad.sum())}")
    assert not bool(bad.any()), (what, int(bad.sum()),
                                 bad.nonzero()[:4].tolist())


def _assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    rel = (err / ref.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e} (rel {rel:.3e}), "
          f"min bound {bound.min().item():.3e}, "
          f"max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all()), (what, (err - bound).max().item())


# ------------------------------------------------ 1. BN backward, exact -----

# (shape, the edge it is there for)
BWD_SHAPES = [
    ((1, 8), "M=1"),
    ((3, 8), "M<nw"),
    ((5, 24), "block255"),
    ((45, 1032), "nw1"),
    ((18, 2048), "cpg256"),
    ((2, 64, 13, 13), "two_trips"),
    ((4, 64, 16, 16), "pow2"),
    ((4096, 16), "pow2"),
    ((6151, 2048), "both_caps"),
    # channels_last twins (shape_mc's 4-D branch)
    ((1, 8, 1, 1), "M=1"),
    ((1, 8, 3, 1), "M<nw"),
    ((1, 24, 1, 5), "block255"),
    ((1, 1032, 5, 9), "nw1"),
    ((2, 2048, 3, 3), "cpg256"),
    ((1, 16, 64, 64), "pow2"),
    ((1, 2048, 6151, 1), "both_caps"),
]
BWD_MODES = ["plain", "relu", "relu_dresid", "relu_eval"]
BWD_PARAMS = [(s, m) for s, _ in BWD_SHAPES for m in BWD_MODES]

POOL2_SHAPES = [
    ((2, 8, 2, 2), "M<nw"),
    ((1, 24, 4, 6), "block255"),
    ((2, 64, 16, 16), "pow2"),
    ((1, 1032, 92, 90), "pool2_dx_cap"),
]


def _pool2_geom(shape):
    N, C, H, W = shape
    Mp = N * (H // 2) * (W // 2)
    g = _geom(4 * Mp, C)
    g["Mp"] = Mp
    g["S"] = max(1, min(1024, Mp // (4 * g["nw"])))
    g["dxblocks"] = max(1, min(2048, Mp // g["nw"]))
    return g


def test_shape_tables_reach_what_they_claim():
    """Each row of the tables reaches the edge it names, by the mirrored
    host geometry."""
    for shape, edge in BWD_SHAPES:
        M, C = _mc(shape)
        g = _geom(M, C)
        part = _trip_counts(M, g["S"] * g["nw"])
        dx = _trip_counts(M, g["dxblocks"] * g["nw"])
        if edge == "M=1":
            assert M == 1
        elif edge == "M<nw":
            assert 1 < M < g["nw"]
        elif edge == "block255":
            assert g["block"] == 255 and g["block"] % 64
        elif edge == "nw1":
            assert g["nw"] == 1 and g["cpg"] == 129 and g["S"] == 11
            assert M % g["S"] and 5 in part      # two trips plus the tail
        elif edge == "cpg256":
            assert g["cpg"] == 256 and g["nw"] == 1
        elif edge == "two_trips":
            assert g["S"] == 2 and 5 in part     # two trips plus the tail
            assert 3 in dx                        # one trip plus the tail
        elif edge == "pow2":
            assert _pow2(M) and M <= 4096
        elif edge == "both_caps":
            assert g["S"] == 1024 and M // (4 * g["nw"]) > 1024
            assert g["dxblocks"] == 2048 and M // (2 * g["nw"]) > 2048
            assert part == {7, 6}     # three trips + tail (7 rows' worth)
            assert M - 6 * g["S"] * g["nw"] == 7
            assert dx == {4, 3}       # second trip for 7 rows, else tail
            assert M - 3 * g["dxblocks"] * g["nw"] == 7
        else:
            raise AssertionError(edge)
    # the table as a whole holds every edge of the list
    assert {e for _, e in BWD_SHAPES} == {
        "M=1", "M<nw", "block255", "nw1", "cpg256", "two_trips", "pow2",
        "both_caps"}
    twins = {e for s, e in BWD_SHAPES if len(s) == 4}
    assert twins >= {"M=1", "M<nw", "block255", "nw1", "cpg256", "pow2",
                     "both_caps", "two_trips"}
    for shape, edge in POOL2_SHAPES:
        g = _pool2_geom(shape)
        if edge == "M<nw":
            assert g["Mp"] < g["nw"]
        elif edge == "block255":
            assert g["block"] == 255
        elif edge == "pow2":
            assert _pow2(4 * g["Mp"]) and 4 * g["Mp"] <= 4096
        elif edge == "pool2_dx_cap":
            assert g["Mp"] // g["nw"] > 2048 and g["dxblocks"] == 2048
            assert g["S"] > 1 and g["Mp"] % (g["S"] * g["nw"])
    # apply: unrolled trip + tail, both channel groups of a trip differ
    for (M, C), want in APPLY_BIG.items():
        g = _geom(M, C)
        assert g["tv"] > g["stride"] == 2 ** 20
        assert _trip_counts(g["tv"], g["stride"]) == want["counts"]
        assert (g["stride"] % g["cpg"] != 0) == want["cv_differs"]
    for shape, _ in BWD_SHAPES:
        M, C = _mc(shape)
        if (M, C) not in APPLY_BIG:
            assert _geom(M, C)["tv"] <= _geom(M, C)["stride"]   # tail only


@functools.lru_cache(maxsize=None)
def _bwd_case(M, C):
    x = _ints((M, C), -4, 4, "bwd x")
    dy = _ints((M, C), -2, 2, "bwd dy")
    mean = _choice([-1.0, 0.0, 1.0], C, "bwd mean")
    invstd = _choice([0.5, 1.0, 2.0], C, "bwd invstd")
    gamma = _choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, "bwd gamma")
    bits = torch.randint(0, 2, (M, C), generator=_gen(M, C, "bits")).bool()
    return x, dy, mean, invstd, gamma, bits


def _check_bwd(M, x, dy_eff, mean, invstd, gamma, eval_stats,
               dx, dgamma, dbeta, what):
    """Shared by bn_bwd and bn_bwd_pool2: everything is [M, C] float64."""
    xhat = (x - mean) * invstd
    t2 = dy_eff * xhat
    assert dy_eff.abs().sum(0).max().item() < 2 ** 23
    assert t2.abs().sum(0).max().item() < 2 ** 23
    dbeta_ref, dgamma_ref = dy_eff.sum(0), t2.sum(0)
    assert torch.equal(dbeta.cpu().double(), dbeta_ref), what
    assert torch.equal(dgamma.cpu().double(), dgamma_ref), what
    ca = gamma * invstd
    if eval_stats:
        assert torch.equal(dx, _bf(ca * dy_eff)), what
        return
    cb, cc = dbeta_ref / M, dgamma_ref / M
    prod = xhat * cc
    ref = ca * (dy_eff - cb - prod)
    if _pow2(M) and M <= 4096:
        for t in (cb, cc, prod, dy_eff - cb, dy_eff - cb - prod, ref):
            assert _fp32_exact(t)
        assert torch.equal(dx, _bf(ref)), what
    else:
        e = 3 * U * SLACK * ca.abs() * (dy_eff.abs() + cb.abs() + prod.abs())
        _assert_band(dx, ref, e, what)


@pytest.mark.parametrize("shape,mode", BWD_PARAMS,
                         ids=[f"{_sid(s)}-{m}" for s, m in BWD_PARAMS])
def test_bn_bwd_exact(shape, mode):
    M, C = _mc(shape)
    x, dy, mean, invstd, gamma, bits = _bwd_case(M, C)
    relu = mode != "plain"
    dresid = mode == "relu_dresid"
    eval_stats = mode == "relu_eval"
    dy_eff = dy * bits if relu else dy
    mask = _pack_mask(bits).to(DEV) if relu \
        else torch.empty(0, dtype=torch.uint8, device=DEV)
    assert mask.shape == ((M, C // 8) if relu else (0,))
    out = ext.bn_bwd(_dev(x, shape), _dev(dy, shape), _f32(gamma),
                     _f32(mean), _f32(invstd), mask, relu, dresid, None,
                     eval_stats)
    assert len(out) == (4 if dresid else 3)
    assert out[0].shape == tuple(shape) and out[0].dtype == BF
    if len(shape) == 4:
        assert out[0].is_contiguous(memory_format=torch.channels_last)
    if dresid:
        assert out[3].shape == tuple(shape)
        assert torch.equal(_rows(out[3]), dy_eff)
    _check_bwd(M, x, dy_eff, mean, invstd, gamma, eval_stats,
               _rows(out[0]), out[1], out[2], f"bn_bwd {shape} {mode}")


@functools.lru_cache(maxsize=None)
def _pool2_case(shape):
    N, C, H, W = shape
    Ho, Wo = H // 2, W // 2
    x = _ints((N * H * W, C), -4, 4, "p2 x")
    dyp = _ints((N, Ho, Wo, C), -2, 2, "p2 dy")
    code = torch.randint(0, 8, (N, Ho, Wo, C),
                         generator=_gen(shape, "p2 code"))
    # dy_eff at full resolution: dy at window position (code & 3) when
    # bit 2 is set, zero elsewhere
    on = ((code & 4) != 0).double() * dyp
    win = F.one_hot(code & 3, 4).double() * on.unsqueeze(-1)
    dy_eff = win.view(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3) \
        .reshape(N * H * W, C)
    return x, dyp, code.to(torch.uint8), dy_eff


@pytest.mark.parametrize("shape", [s for s, _ in POOL2_SHAPES], ids=_sid)
def test_bn_bwd_pool2_exact(shape):
    N, C, H, W = shape
    M = N * H * W
    x, dyp, code, dy_eff = _pool2_case(shape)
    _, _, mean, invstd, gamma, _ = _bwd_case(1, C)
    dyd = dyp.to(BF).permute(0, 3, 1, 2).to(DEV)
    assert dyd.is_contiguous(memory_format=torch.channels_last)
    dx, dgamma, dbeta = ext.bn_bwd_pool2(
        _dev(x, shape), dyd, _f32(gamma), _f32(mean), _f32(invstd),
        code.to(DEV))
    assert dx.shape == tuple(shape)
    assert dx.is_contiguous(memory_format=torch.channels_last)
    _check_bwd(M, x, dy_eff, mean, invstd, gamma, False, _rows(dx), dgamma,
               dbeta, f"bn_bwd_pool2 {shape}")


# -------------------------------------------- 2. BN forward statistics ------

def _stat_bounds(x, exact_sums):
    """Per-channel float64 truths and the section-2 bounds for [M, C] x."""
    M, C = x.shape
    g = _geom(M, C)
    a1, s2 = x.abs().sum(0), (x * x).sum(0)
    mean, msq = x.sum(0) / M, s2 / M
    var = (msq - mean * mean).clamp_min(0)
    if exact_sums:
        assert a1.max().item() < 2 ** 24 and s2.max().item() < 2 ** 24
        gam = 0.0
    else:
        gam = (g["L"] + g["T"]) * U
        assert g["L"] + g["T"] < 5792
    udiv = 0.0 if (exact_sums and _pow2(M)) else U
    e_mean = gam * a1 / M + udiv * mean.abs()
    e_msq = gam * msq + udiv * msq
    e_var = (e_msq + 2 * mean.abs() * e_mean + e_mean ** 2
             + 3 * U * (msq + mean * mean)) * SLACK
    if M == 1 and exact_sums:
        # mean = x, msq = x*x = fl(mean*mean): the difference is exactly 0
        e_var = torch.zeros_like(var)
    lo_a = (var + EPS32 - e_var) * (1 - U)
    hi_a = (var + EPS32 + e_var) * (1 + U)
    assert lo_a.min().item() > 0
    inv = (var + EPS32) ** -0.5
    inv_lo = hi_a ** -0.5 * (1 - 2 * R_RSQRT * U * SLACK)
    inv_hi = lo_a ** -0.5 * (1 + 2 * R_RSQRT * U * SLACK)
    if M > 1:
        unb = var * M / (M - 1)
        e_unb = (e_var * M / (M - 1) + 2 * U * unb) * SLACK
    else:
        unb, e_unb = var, e_var
    return dict(mean=mean, var=var, e_mean=e_mean, e_var=e_var, inv=inv,
                inv_lo=inv_lo, inv_hi=inv_hi, unb=unb, e_unb=e_unb,
                gamma_s=gam)


def _check_stats(st, sm, si, rm, rv, rm0, rv0, what):
    """save_mean, save_invstd and the blended running statistics."""
    sm, si = sm.cpu().double(), si.cpu().double()
    rm, rv = rm.cpu().double(), rv.cpu().double()
    if bool((st["e_mean"] == 0).all()):
        assert torch.equal(sm, st["mean"]), what
    else:
        _assert_within(sm, st["mean"], st["e_mean"] * SLACK, what + " mean")
    inside = (si >= st["inv_lo"]) & (si <= st["inv_hi"])
    rel = ((si - st["inv"]).abs() / st["inv"]).max().item()
    width = ((st["inv_hi"] - st["inv_lo"]) / st["inv"]).max().item() / 2
    print(f"{what} invstd: max rel err {rel:.3e} = {rel / U:.2f} u, "
          f"widest bound {width:.3e} = {width / U:.1f} u")
    assert bool(inside.all()), (what, "invstd", int((~inside).sum()))
    a1, m = ONE_MINUS_MOM32, MOM32
    mean_mag = st["mean"].abs() + st["e_mean"]
    e_rm = (m * st["e_mean"]
            + 2 * U * SLACK * ((a1 * rm0).abs() + m * mean_mag))
    _assert_within(rm, a1 * rm0 + m * st["mean"], e_rm, what + " run_mean")
    e_rv = (m * st["e_unb"]
            + 2 * U * SLACK * ((a1 * rv0).abs()
                               + m * (st["unb"] + st["e_unb"])))
    _assert_within(rv, a1 * rv0 + m * st["unb"], e_rv, what + " run_var")
    rel_var = (st["e_var"] / st["var"].clamp_min(1e-300)).max().item()
    print(f"{what}: variance bound / var, worst channel {rel_var:.3e}")


def _run_stats(C, key):
    """non-trivial initial running statistics: an overwrite instead of a
    blend, or a swapped pair, cannot pass"""
    rm0 = _randn((C,), key, "rm0").double()
    rv0 = _randn((C,), key, "rv0").double().abs() + 0.5
    return rm0, rv0


STAT_INT_SHAPES = [(1, 8), (2, 8), (256, 24), (4, 64, 16, 16), (4096, 16),
                   (32, 1032), (16, 2048)]


@pytest.mark.parametrize("shape", STAT_INT_SHAPES, ids=_sid)
def test_bn_fwd_stats_integer(shape):
    M, C = _mc(shape)
    assert _pow2(M)
    x = _ints((M, C), -4, 4, "stat x")
    st = _stat_bounds(x, True)
    gamma = _choice([0.5, 1.0, 2.0], C, "stat g")
    beta = _choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, "stat b")
    rm0, rv0 = _run_stats(C, "int")
    rm, rv = _f32(rm0), _f32(rv0)
    rm0, rv0 = rm.cpu().double(), rv.cpu().double()
    y, sm, si, mask = ext.bn_fwd_train(_dev(x, shape), _f32(gamma),
                                       _f32(beta), rm, rv, MOM, EPS, False)
    assert mask.numel() == 0 and y.shape == tuple(shape)
    assert bool((st["e_mean"] == 0).all())
    _check_stats(st, sm, si, rm, rv, rm0, rv0, f"int {shape}")
    if M == 1:
        # biased variance (the M > 1 guard): var = 0, nothing to blend in
        assert torch.equal(st["unb"], torch.zeros(C, dtype=F64))
        # y = fl(x*sc + fl(beta - fl(x*sc))) is beta plus at most three
        # roundings of magnitude |x*sc| + |beta|; beta is a power of two
        # times +-1, the bf16 spacing just below it is |beta| * 2^-8, and a
        # quarter of that is asserted here
        err = 3 * U * (4 * gamma * st["inv_hi"] + beta.abs())
        assert bool((err < beta.abs() * 2.0 ** -10).all())
        assert torch.equal(_rows(y), beta.expand(1, C))


@pytest.mark.parametrize("S", [1, 3, 70])
def test_bn_fwd_pre_stats_integer(S):
    """Statistics handed in as an exact [2][C][S] slab; S = 70 is no
    multiple of the 64-lane sweep."""
    M, C = 256, 24
    x = _ints((M, C), -4, 4, "stat x")
    st = _stat_bounds(x, True)
    parts = torch.tensor_split(x, S)
    slab = torch.stack([torch.stack([p.sum(0) for p in parts], 1),
                        torch.stack([(p * p).sum(0) for p in parts], 1)])
    assert slab.shape == (2, C, S)
    gamma = _choice([0.5, 1.0, 2.0], C, "stat g")
    beta = _randn_bf16((C,), "stat b")
    rm0, rv0 = _run_stats(C, "pre")
    rm, rv = _f32(rm0), _f32(rv0)
    rm0, rv0 = rm.cpu().double(), rv.cpu().double()
    _, sm, si, _ = ext.bn_fwd_train(_dev(x, (M, C)), _f32(gamma), _f32(beta),
                                    rm, rv, MOM, EPS, False, None,
                                    slab.float().contiguous().to(DEV))
    _check_stats(st, sm, si, rm, rv, rm0, rv0, f"pre_stats S={S}")


STAT_RAND_SHAPES = [(5, 24), (2, 64, 13, 13), (45, 1032), (6151, 2048)]


@pytest.mark.parametrize("ratio", [0, 4, 32])
@pytest.mark.parametrize("shape", STAT_RAND_SHAPES, ids=_sid)
def test_bn_fwd_stats_random(shape, ratio):
    M, C = _mc(shape)
    std = 0.5 + _randn((C,), "std").abs()
    x = ((_randn((M, C), "rand x") + float(ratio)) * std).to(BF).double()
    st = _stat_bounds(x, False)
    rm0, rv0 = _run_stats(C, "rand")
    rm, rv = _f32(rm0), _f32(rv0)
    rm0, rv0 = rm.cpu().double(), rv.cpu().double()
    _, sm, si, _ = ext.bn_fwd_train(_dev(x, shape), _f32(torch.ones(C)),
                                    _f32(torch.zeros(C)), rm, rv, MOM, EPS,
                                    False)
    _check_stats(st, sm, si, rm, rv, rm0, rv0,
                 f"rand {shape} mean/std={ratio}")
    # the kernel's own variance, recovered from save_invstd (characterised,
    # not asserted beyond the interval above)
    var_k = si.cpu().double() ** -2 - EPS32
    err = ((var_k - st["var"]).abs() / st["var"]).max().item()
    print(f"rand {shape} mean/std={ratio}: measured |var_k - var| / var, "
          f"worst channel {err:.3e}")


# ------------------------------------------------------- 3. BN apply --------

def _apply_ref(x, resid, gamma, beta, mean, e_mean, inv, inv_lo, inv_hi):
    """float64 truth and the section-3 error bound, [M, C]."""
    sc = gamma * inv
    e_sc = gamma.abs() * (torch.maximum(inv_hi - inv, inv - inv_lo)
                          + U * inv_hi)
    ms = (mean.abs() + e_mean) * (sc.abs() + e_sc)
    e_sh = (mean.abs() * e_sc + e_mean * (sc.abs() + e_sc)
            + 2 * U * (beta.abs() + ms))
    ref = (x - mean) * sc + beta
    mag = x.abs() * (sc.abs() + e_sc) + ms + beta.abs() + e_sh
    if resid is not None:
        ref = ref + resid
        mag = mag + resid.abs()
    e = (x.abs() * e_sc + e_sh + 2 * U * mag) * SLACK
    k = (e_sc / (U * sc.abs().clamp_min(1e-300))).max().item() + 4
    return ref, e, k


def _check_apply(y, mask, ref, e, relu, C, what):
    _assert_band(y, ref, e, what, relu=relu)
    if not relu:
        return
    M = ref.shape[0]
    sure = ref.abs() > e
    left_out = 1.0 - sure.double().mean().item()
    print(f"{what}: left-out share {left_out:.3e}")
    assert left_out <= 1e-3
    assert bool(((y > 0) == (ref > 0))[sure].all()), what
    if mask is not None:
        assert mask.shape == (M, C // 8) and mask.dtype == torch.uint8
        bits = _unpack_mask(mask, C)
        assert bool((bits == (ref > 0))[sure].all()), what


def _apply_inputs(M, C, resid):
    x = _ints((M, C), -4, 4, "apply x")
    gamma = _randn((C,), "apply g").double()
    beta = _randn((C,), "apply b").double()
    r = _randn_bf16((M, C), "apply r") if resid else None
    return x, gamma, beta, r


def _run_train(shape, relu, resid):
    M, C = _mc(shape)
    x, gamma, beta, r = _apply_inputs(M, C, resid)
    st = _stat_bounds(x, True)
    rm, rv = _f32(torch.zeros(C)), _f32(torch.ones(C))
    y, sm, si, mask = ext.bn_fwd_train(
        _dev(x, shape), _f32(gamma), _f32(beta), rm, rv, MOM, EPS, relu,
        _dev(r, shape) if resid else None)
    assert y.shape == tuple(shape) and y.dtype == BF
    gamma, beta = gamma.float().double(), beta.float().double()
    ref, e, k = _apply_ref(x, r, gamma, beta, st["mean"], st["e_mean"],
                           st["inv"], st["inv_lo"], st["inv_hi"])
    what = f"train {shape} relu={relu} resid={resid}"
    print(f"{what}: k = {k:.1f}")
    if not relu:
        assert mask.numel() == 0
    _check_apply(_rows(y), mask if relu else None, ref, e, relu, C, what)


def _run_eval(shape, relu, resid, with_mask):
    M, C = _mc(shape)
    x, gamma, beta, r = _apply_inputs(M, C, resid)
    rm0 = _randn((C,), "eval rm").float()
    rv0 = _randn((C,), "eval rv").float().abs() + 0.25
    args = (_dev(x, shape), _f32(gamma), _f32(beta), rm0.to(DEV),
            rv0.to(DEV), EPS, relu, _dev(r, shape) if resid else None)
    if with_mask:
        y, mask = ext.bn_fwd_eval_mask(*args)
        if not relu:
            assert mask.numel() == 0
    else:
        y, mask = ext.bn_fwd_eval(*args), None
    assert y.shape == tuple(shape) and y.dtype == BF
    gamma, beta = gamma.float().double(), beta.float().double()
    a = rv0.double() + EPS32
    inv = a ** -0.5
    inv_lo = (a * (1 + U)) ** -0.5 * (1 - 2 * R_RSQRT * U * SLACK)
    inv_hi = (a * (1 - U)) ** -0.5 * (1 + 2 * R_RSQRT * U * SLACK)
    ref, e, k = _apply_ref(x, r, gamma, beta, rm0.double(),
                           torch.zeros(C, dtype=F64), inv, inv_lo, inv_hi)
    what = f"eval{'_mask' if with_mask else ''} {shape} relu={relu} " \
           f"resid={resid}"
    print(f"{what}: k = {k:.1f}")
    assert k <= 2 * R_RSQRT + 6
    _check_apply(_rows(y), mask if (relu and with_mask) else None, ref, e,
                 relu, C, what)


APPLY_SMALL = [s for s, _ in BWD_SHAPES if _mc(s)[0] * _mc(s)[1] < 10 ** 6]
# (M, C) past the 4096-block cap: iteration counts per thread and whether
# the two vectors of an unrolled trip sit in different channel groups
APPLY_BIG = {
    (6151, 2048): dict(counts={2, 1}, cv_differs=False),
    (524289, 24): dict(counts={2, 1}, cv_differs=True),
    (2 ** 20 + 3, 24): dict(counts={4, 3}, cv_differs=True),
}


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", APPLY_SMALL, ids=_sid)
def test_bn_apply_small(shape, relu, resid):
    _run_train(shape, relu, resid)
    _run_eval(shape, relu, resid, with_mask=False)
    _run_eval(shape, relu, resid, with_mask=True)


def test_bn_apply_train_both_caps():
    _run_train((6151, 2048), True, True)


def test_bn_apply_train_unrolled_trip_cv3():
    """tv = 1.5 * 2^20 + 3 with Cv = 3: a third of the threads take the
    unrolled trip, and 2^20 % 3 = 1 puts its two vectors in different
    channel groups."""
    _run_train((524289, 24), True, True)


def test_bn_apply_eval_two_unrolled_trips():
    """tv = 3 * 2^20 + 9: nine threads take a second unrolled trip."""
    _run_eval((2 ** 20 + 3, 24), True, False, with_mask=True)


# ---------------------------------------------------------- 4. pooling ------

def _nchw(t):
    """[N, H, W, C] or channels_last device tensor -> NCHW-contiguous CPU
    float64"""
    return t.cpu().double().contiguous()


def _pool_ref(x, ks, st, pad):
    """float64 CPU max-pool: y, window-local argmax codes [N, Ho, Wo, C],
    and dx for ``dy``."""
    N, C, H, W = x.shape
    xr = x.clone().requires_grad_(True)
    y, flat = F.max_pool2d(xr, ks, st, pad, return_indices=True)
    Ho, Wo = y.shape[2:]
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    kh = flat // W - (ho * st - pad)
    kw = flat % W - (wo * st - pad)
    assert int(kh.min()) >= 0 and int(kh.max()) < ks
    assert int(kw.min()) >= 0 and int(kw.max()) < ks
    code = (kh * ks + kw).permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    dy = _ints(tuple(y.shape), -2, 2, "pool dy", ks, st, pad)
    y.backward(dy)
    return y.detach(), code, dy, xr.grad


def _pool_x(N, C, H, W):
    x = _ints((N, C, H, W), -3, 3, "pool x")
    return x


def _cl(t64):
    return t64.to(BF).to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("C", [8, 24, 128])
def test_maxpool2x2_exact(C):
    for H, W in [(2, 2), (2, 6), (6, 4), (24, 24)]:
        N = 3
        x = _pool_x(N, C, H, W)
        y_ref, code_ref, dy, dx_ref = _pool_ref(x, 2, 2, 0)
        y, idx = ext.maxpool2x2_fwd(_cl(x))
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(_nchw(y), y_ref), (C, H, W)
        assert idx.shape == (N, H // 2, W // 2, C)
        assert idx.dtype == torch.uint8
        assert torch.equal(idx.cpu(), code_ref), (C, H, W)
        dx = ext.maxpool2x2_bwd(_cl(dy), idx, H, W)
        assert dx.shape == x.shape
        assert torch.equal(_nchw(dx), dx_ref), (C, H, W)
    # a quarter of the 2x2 windows hold their maximum more than once
    # (measured 27 %; 52 % of the 3x3 windows)
    x = _pool_x(3, C, 24, 24)
    win = x.view(3, C, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5) \
        .reshape(3, C, 12, 12, 4)
    tied = ((win == win.max(-1, keepdim=True).values).sum(-1) > 1)
    assert tied.double().mean().item() > 0.2


POOL_CFGS = [(3, 2, 1), (3, 1, 1), (2, 2, 0), (5, 3, 2), (2, 1, 0)]
POOL_EXTENTS = [(7, 9), (4, 4), (6, 8)]


def _uncovered(H, ks, st, pad):
    """rows (or columns) past the last window"""
    Ho = (H + 2 * pad - ks) // st + 1
    return list(range((Ho - 1) * st + ks - pad, H))


def test_pool_tables_reach_what_they_claim():
    for ks, st, pad in POOL_CFGS:
        if st > 1:
            assert any((H + 2 * pad - ks) % st for H, _ in POOL_EXTENTS)
            assert any((W + 2 * pad - ks) % st for _, W in POOL_EXTENTS)
    assert _uncovered(7, 2, 2, 0) == [6] and _uncovered(9, 2, 2, 0) == [8]
    assert any(st < ks for ks, st, _ in POOL_CFGS)       # overlapping
    assert (7, 9) in POOL_EXTENTS                          # odd, H != W


@pytest.mark.parametrize("cfg", POOL_CFGS, ids=lambda c: "k%ds%dp%d" % c)
def test_maxpool_general_exact(cfg):
    ks, st, pad = cfg
    for H, W in POOL_EXTENTS:
        for C in (8, 24):
            N = 2
            x = _pool_x(N, C, H, W)
            y_ref, code_ref, dy, dx_ref = _pool_ref(x, ks, st, pad)
            y, idx = ext.maxpool_fwd(_cl(x), ks, st, pad)
            assert torch.equal(_nchw(y), y_ref), (cfg, H, W, C)
            assert idx.shape == code_ref.shape
            assert torch.equal(idx.cpu(), code_ref), (cfg, H, W, C)
            dx = ext.maxpool_bwd(_cl(dy), idx, H, W, ks, st, pad)
            assert dx.shape == x.shape
            got = _nchw(dx)
            assert torch.equal(got, dx_ref), (cfg, H, W, C)
            for h in _uncovered(H, ks, st, pad):
                assert not bool(got[:, :, h, :].any())
            for w in _uncovered(W, ks, st, pad):
                assert not bool(got[:, :, :, w].any())
            if cfg == (2, 2, 0) and H % 2 == 0 and W % 2 == 0:
                y2, idx2 = ext.maxpool2x2_fwd(_cl(x))
                assert torch.equal(y2, y) and torch.equal(idx2, idx)
                assert torch.equal(ext.maxpool2x2_bwd(_cl(dy), idx2, H, W),
                                   dx)


@pytest.mark.parametrize("C", [8, 24, 2048])
def test_global_avgpool(C):
    g = _geom(1, C)
    assert {8: g["nw"] == 256, 24: g["block"] == 255,
            2048: g["nw"] == 1}[C]
    N = 3
    for H, W in [(1, 1), (2, 2), (8, 8), (7, 7)]:
        HW = H * W
        x = _ints((N, C, H, W), -3, 3, "gap x")
        dy = _ints((N, C), -3, 3, "gap dy", HW)
        y = ext.global_avgpool_fwd(_cl(x))
        dx = ext.global_avgpool_bwd(dy.to(BF).to(DEV), H, W)
        assert y.shape == (N, C) and dx.shape == x.shape
        assert dx.is_contiguous(memory_format=torch.channels_last)
        y, dx = y.cpu().double(), _nchw(dx)
        y_ref = x.sum((2, 3)) / HW
        dx_ref = (dy / HW).view(N, C, 1, 1).expand(N, C, H, W)
        if _pow2(HW):
            assert _fp32_exact(y_ref) and _fp32_exact(dx_ref)
            assert torch.equal(y, _bf(y_ref)), (C, HW)
            assert torch.equal(dx, _bf(dx_ref)), (C, HW)
        else:
            _assert_band(y, y_ref, 2 * U * SLACK * y_ref.abs(),
                         f"gap fwd C={C} HW={HW}")
            _assert_band(dx, dx_ref, 2 * U * SLACK * dx_ref.abs(),
                         f"gap bwd C={C} HW={HW}")


# ---------------------------------------------------- 5. cross-entropy ------

CE_PATHS = [("bf16", 10), ("bf16", 63), ("fp32", 10),
            ("bf16", 64), ("bf16", 520), ("bf16", 1000)]
CE_BATCHES = [1, 3, 5, 255, 257, 1030]


def _ce_wave(dtype, C):
    return dtype == "bf16" and C % 8 == 0 and C >= 64


@functools.lru_cache(maxsize=None)
def _ce_case(dtype, C, B):
    x = _randn((B, C), "ce x", dtype)
    t = torch.randint(0, C, (B,), generator=_gen(B, C, "ce t"))
    if B > 2:
        x[2] *= 80.0                 # overflows without the max shift
    if B > 3:
        x[3, C - 1] = 30.0           # the maximum in the last chunk
    if B > 4:
        x[4] = x[4] * 80.0 - 80.0
    x = (x.to(BF) if dtype == "bf16" else x.float()).double()
    t[0] = 0
    t[B - 1] = C - 1 if B > 1 else 0
    if B > 2:
        t[1] = int(x[1].argmax())
    return x, t


def _ce_bounds(x, t, wave):
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
    row = lse - x.gather(1, t.view(B, 1)).squeeze(1)
    e_row = e_lse + U * SLACK * row.abs()
    loss = row.mean()
    e_loss = e_row.mean() + (_cdiv(B, 256) + 9) * U * SLACK * row.abs().mean()
    return lse, e_lse, loss, e_loss


@pytest.mark.parametrize("B", CE_BATCHES)
@pytest.mark.parametrize("dtype,C", CE_PATHS)
def test_cross_entropy(dtype, C, B):
    x, t = _ce_case(dtype, C, B)
    wave = _ce_wave(dtype, C)
    assert wave == (C in (64, 520, 1000))
    lse_ref, e_lse, loss_ref, e_loss = _ce_bounds(x, t, wave)
    xd = x.to(BF if dtype == "bf16" else torch.float32).to(DEV)
    td = t.to(DEV)
    loss, lse = ext.ce_fwd(xd, td)
    assert lse.shape == (B,) and lse.dtype == torch.float32
    assert loss.dim() == 0
    what = f"ce {dtype} B={B} C={C}"
    _assert_within(lse.cpu().double(), lse_ref, e_lse, what + " lse")
    _assert_within(loss.cpu().double(), loss_ref, e_loss, what + " loss")

    dloss = 0.37
    dl = ext.ce_bwd(xd, td, lse, torch.tensor(dloss, device=DEV))
    assert dl.shape == (B, C) and dl.dtype == xd.dtype
    g = float(torch.tensor(dloss, dtype=torch.float32)) / B
    z = x - lse_ref.view(B, 1)
    p = torch.exp(z)
    oh = F.one_hot(t, C).double()
    ref = (p - oh) * g
    e = g * SLACK * (p * (e_lse.view(B, 1) + U * z.abs() + 2 * R_EXP * U)
                     + U * (3 * (p - oh).abs()).clamp_max(1.0)) + TINY
    got = dl.cpu().double()
    if dtype == "bf16":
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


def _first_max(x):
    C = x.shape[1]
    hit = x == x.max(1, keepdim=True).values
    return torch.where(hit, torch.arange(C).expand_as(x), C).min(1).values


@pytest.mark.parametrize("C", [10, 64, 1000])
def test_argmax_correct_ties(C):
    """Integer logits, the maximum twice per row: in neighbouring chunks
    (every lane boundary), and in a later chunk of a lower lane against an
    earlier chunk of a higher lane (the shuffle tree must prefer the
    smaller index, not the lower lane)."""
    pairs = [(a, a + 1) for a in range(C - 1)]
    pairs += [(a, b) for a in range(0, C - 1, 3)
              for b in range(a + 2, C, max(1, C // 7))]
    if C >= 1000:
        pairs += [(8 * (lane + 1) + j, 8 * (lane + 64) + (7 - j))
                  for lane in range(0, 60) for j in (0, 7)]
    B = len(pairs)
    x = _ints((B, C), -3, 3, "argmax x")
    for r, (a, b) in enumerate(pairs):
        x[r, a] = x[r, b] = 5.0
    first = _first_max(x)
    assert torch.equal(first, torch.tensor([a for a, _ in pairs]))
    xd = x.to(BF).to(DEV)
    second = torch.tensor([b for _, b in pairs])
    mixed = torch.where(torch.arange(B) % 2 == 0, first, second)
    for name, t in (("first", first), ("second", second), ("mixed", mixed)):
        want = int((first == t).sum())
        got = int(ext.argmax_correct(xd, t.to(DEV)))
        assert got == want, (C, name, got, want)


# ------------------------------------------- 6. overflow stays visible ------

def _unpoisoned(C, c0):
    return torch.tensor([c for c in range(C) if c != c0])


@pytest.mark.parametrize("poison", [float("inf"), float("nan")],
                         ids=["inf", "nan"])
@pytest.mark.parametrize("fused_pool", [False, True], ids=["bn", "bn_pool2"])
def test_poisoned_channel_reaches_the_overflow_flag(poison, fused_pool):
    """fmaxf(NaN, 0) = 0: the fused ReLU turns a poisoned channel into
    zeros (and clears its mask bits), but xhat is +-inf or NaN there and
    fmaf(0, xhat, acc) poisons dgamma, so amp still skips the step."""
    N, C, H, W = 2, 16, 4, 4
    c0 = 5
    shape = (N, C, H, W)
    x = _randn_bf16((N * H * W, C), "poison x")
    xp = x.clone()
    xp[7, c0] = poison
    gamma = _randn((C,), "poison g").abs().double() + 0.5
    beta = _randn((C,), "poison b").double()
    ho, wo = (H // 2, W // 2) if fused_pool else (H, W)
    dy = _dev(_randn_bf16((N * ho * wo, C), "poison dy"), (N, C, ho, wo))

    def run(xr):
        rm, rv = _f32(torch.zeros(C)), _f32(torch.ones(C))
        xd = _dev(xr, shape)
        if fused_pool:
            y, sm, si, code = ext.bn_fwd_train_pool2(
                xd, _f32(gamma), _f32(beta), rm, rv, MOM, EPS)
            dx, dg, db = ext.bn_bwd_pool2(xd, dy, _f32(gamma), sm, si, code)
        else:
            y, sm, si, mask = ext.bn_fwd_train(
                xd, _f32(gamma), _f32(beta), rm, rv, MOM, EPS, True)
            dx, dg, db = ext.bn_bwd(xd, dy, _f32(gamma), sm, si, mask, True)
        return dict(y=y, dx=dx, dg=dg, db=db, sm=sm, si=si, rm=rm, rv=rv)

    clean, bad = run(x), run(xp)
    assert not bool(torch.isfinite(bad["dg"][c0]))
    assert bool(torch.isfinite(clean["dg"]).all())
    flag = torch.zeros(1, device=DEV)
    ext.multi_tensor_unscale([bad["dg"].clone()], flag, 1.0)
    assert flag.item() == 1.0
    flag = torch.zeros(1, device=DEV)
    ext.multi_tensor_unscale([clean["dg"].clone()], flag, 1.0)
    assert flag.item() == 0.0
    keep = _unpoisoned(C, c0).to(DEV)
    for k in ("y", "dx"):
        assert torch.equal(bad[k].index_select(1, keep),
                           clean[k].index_select(1, keep)), k
    for k in ("dg", "db", "sm", "si", "rm", "rv"):
        assert torch.equal(bad[k][keep], clean[k][keep]), k


# ----------------------------------- measured library-function errors -------

def _ulp32(v64):
    """ulp of the fp32 binade holding |v|"""
    return 2.0 ** (torch.floor(torch.log2(v64.abs())) - 23)


def test_math_function_ulp_errors():
    """rsqrtf, expf and logf against float64, each isolated through an
    entry point that exposes the fp32 result unrounded; R_* is twice the
    measured maximum, rounded up."""
    # rsqrtf: pre_stats with sum = 0 and sq = M*v, M = 2: mean = 0,
    # var = v exactly, save_invstd = rsqrtf(fl(v + eps))
    C, M = 2048, 2
    v = torch.exp(_randn((C,), "rsqrt v") * 3.0).float().clamp(1e-5, 1e3)
    slab = torch.stack([torch.zeros(C), v * M]).view(2, C, 1)
    x = torch.zeros(M, C).to(BF).to(DEV)
    _, sm, si, _ = ext.bn_fwd_train(
        x, _f32(torch.ones(C)), _f32(torch.zeros(C)), _f32(torch.zeros(C)),
        _f32(torch.ones(C)), MOM, EPS, False, None,
        slab.float().contiguous().to(DEV))
    assert not bool(sm.cpu().any())
    a = (v + torch.tensor(EPS, dtype=torch.float32)).double()
    true = a ** -0.5
    r_rsqrt = ((si.cpu().double() - true).abs() / _ulp32(true)).max().item()
    # expf: ce_bwd on fp32 logits with lse = 0, dloss = B (g = 1), a target
    # column that is left out: dlogits = expf(x)
    B, Cc = 4096, 17
    z = (torch.rand(B, Cc, generator=_gen("exp z")) * 110.0 - 100.0).float()
    t = torch.zeros(B, dtype=torch.long)
    dl = ext.ce_bwd(z.to(DEV), t.to(DEV), torch.zeros(B, device=DEV),
                    torch.tensor(float(B), device=DEV))
    true = torch.exp(z.double())[:, 1:]
    got = dl.cpu().double()[:, 1:]
    normal = true > 2.0 ** -126
    r_exp = (((got - true).abs() / _ulp32(true))[normal]).max().item()
    # logf: rows of k zeros and C - k entries of -200 (expf gives 0): the
    # sum is the integer k in any order, lse = logf(k)
    Cw = 1000
    k = torch.arange(1, Cw + 1)
    rows = torch.where(torch.arange(Cw).view(1, Cw) < k.view(Cw, 1), 0.0,
                       -200.0)
    _, lse = ext.ce_fwd(rows.to(BF).to(DEV),
                        torch.zeros(Cw, dtype=torch.long, device=DEV))
    true = torch.log(k.double())
    err = (lse.cpu().double() - true).abs()
    assert err[0].item() == 0.0
    r_log = (err[1:] / _ulp32(true[1:])).max().item()
    print(f"measured ulp errors: rsqrtf {r_rsqrt:.3f}, expf {r_exp:.3f}, "
          f"logf {r_log:.3f}")
    assert r_rsqrt <= R_RSQRT and r_exp <= R_EXP and r_log <= R_LOG
