"""Attention kernels (ops/hip/attn.hip) against float64 attention on the CPU
over the bf16-rounded operands.

Notation: u = 2^-24, hulp(t) = 2^(floor(log2 t) - 8); a bf16 output y of a value
v64 computed with first-order error e must satisfy
|y - v64| <= hulp(|v64| + e) + e, e carrying the factor 1.01 for the dropped
second-order terms; fp32 outputs lie within 1.01 e.  s = q k^T / 8 are the
scaled logits, P = softmax(s), nt = ceil(L / 64) the streamed tiles and
T = 67 nt: at most 64 nt additions in an accumulator (the MFMA chains over
padded tiles) plus, per tile, the rescale by alpha (one multiply, alpha's exp2
within 2u).

Forward, in the kernel's order: s by MFMA over 64 products (66u sum|q k|, as
for every 64-deep product here); t = s C2 with C2 = fl(log2(e) / 8) (2u|s|);
t - m with the running max (u|t - m| <= 2u max|s|); a term that waits in the
accumulator is later multiplied by alpha = exp2(m_old - m_new), whose argument
errs by at most 2u max|s| again.  So a logit errs by
    ds_i = max_j 66u/8 sum_d|q_id k_jd| + 8u max_j|s_ij|
and p_j and the sum l of the fp32 p (taken before P is rounded) each by the
relative ds_i, l by T u more.  p is rounded to bf16 for the second GEMM: round
to nearest on 8 significant bits errs by up to half an ulp, which for a value
just above a power of two is 2^-8 of it (rb below; 2^-9 holds only just below
the next power of two, and p = exp2(t - m) is rounded against the running max,
so its place in the binade is not that of P).  exp2, the division 1 / l and
the multiply by it add 2u + u + u:
    e_o   = (rb + 2 ds_i + (2T + 8) u) sum_j P_ij |v_jd|
    e_lse = ds_i + (T + 4) u + 2u (log L + max_j|s_ij| + |lse|)
(lse = fma(m, ln 2, logf(l)): an error common to all logits moves lse by as
much, logf within 2u, the constant and the fma u each).

Backward.  Both kernels recompute P = exp2(fma(s, C2, -lse log2 e)):
    eP_i = ds_i + e_lse + 2u|lse| + 2u              (relative)
    dP = do v^T by MFMA:  e_dP = 66u sum_d|do_id v_jd|
    delta_i = sum_d do_id o_id from the saved bf16 o, a 16-term fma chain and
    two tree additions:
        e_delta = sum_d|do_id| (hulp(|o| + e_o) + e_o) + 18u sum_d|do_id o_id|
    dS = P (dP - delta):
        e_dS = P (e_dP + e_delta + u(|dP| + |delta|)) + |dS| (eP_i + u)
    and dS is rounded to bf16, rb (|dS| + e_dS) =: r_dS, before
    dq_id = 1/8 sum_j dS_ij k_jd:  e = 1/8 (sum_j (e_dS + r_dS)|k| + T u sum_j|dS k|)
    dk_jd = 1/8 sum_i dS_ij q_id:  the same against |q|
    dv_jd = sum_i P_ij do_id, P rounded to bf16:
        e = sum_i (rb + eP_i) P_ij |do_id| + T u sum_i P_ij |do_id|
The factors 1/8 are exact.

Uniform attention (q = 0, integer v): every p is 1, l = L and sum v are exact,
o = fl(fl(1 / L) sum v): e = 2u|v64|; lse = logf(L): 2u log L + u.

One-hot attention: key j carries 16 in channels j % 14 and 14 + j // 14,
query i the code of its target t(i) = (7i + 3) % L: the target's logit is 64,
a half match 32, the rest 0; the others weigh at most e^-32 each, L e^-32 < u
in all, so o[i] is v[t(i)] to the bit for |v| in [0.5, 1.5].  dv[j] is the
integer sum of the do rows that target j: to the bit where that sum is not 0,
and within L e^-32 max|do| where no row targets j.  Where rows target j and
their integers cancel to 0 the result is not 0: the MFMA aligns its addends to
the largest one, so the others' e^-32 weights leave a residue at the largest
addend's last place (measured: 2^-22 against addends of 4); there dv must lie
within the accumulation term T u sum_i P_ij |do_id| of the bound above.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RB = 2.0 ** -8      # unit roundoff of bf16
BF = torch.bfloat16
F64 = torch.float64
CL = torch.channels_last

if torch.cuda.is_available():
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops import functional as F_ops
    from ddp_tricks_amd.ops.optim import FusedAdamW
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

# (N, heads, H, W): L = 1; 49 one partial tile; 64 exactly one; 65 one row
# into the second; 196 four tiles with a tail of 4
CASES = [(1, 1, 1, 1), (2, 3, 1, 1), (2, 3, 7, 7), (1, 1, 8, 8), (2, 3, 8, 8),
         (1, 3, 5, 13), (2, 1, 13, 5), (2, 1, 14, 14), (1, 3, 14, 14)]


def _bf(t):
    return t.to(BF).to(F64)


def _hulp(t):
    return torch.exp2(torch.floor(torch.log2(t.clamp_min(1e-300))) - 8)


def _within(got, ref, e):
    e = 1.01 * e
    assert bool(((got - ref).abs() <= _hulp(ref.abs() + e) + e).all())


def _grid(t, H, W):
    """[N, heads, L, 64] float64 -> device bf16 channels_last [N, 64 heads, H, W]"""
    N, h, L, d = t.shape
    return (t.transpose(1, 2).reshape(N, H, W, h * d).permute(0, 3, 1, 2)
            .to(BF).contiguous(memory_format=CL).to(DEV))


def _heads(t, h):
    """device [N, 64 h, H, W] -> [N, h, L, 64] float64 on the CPU"""
    N, C, H, W = t.shape
    return (t.permute(0, 2, 3, 1).reshape(N, H * W, h, 64).transpose(1, 2)
            .cpu().to(F64))


def _check(q, k, v, do, H, W, dtype=None):
    """Holds o, lse, dq, dk, dv for float64 operands [N, heads, L, 64] (bf16
    values) to the docstring's bounds; through the bindings, or with `dtype`
    through functional.attention2d on inputs of that dtype.  Returns (o, dv)
    as [N, heads, L, 64] float64."""
    N, h, L, _ = q.shape
    T = 67 * (-(-L // 64))
    s = q @ k.mT / 8
    P = torch.softmax(s, -1)
    lse64 = torch.logsumexp(s, -1, keepdim=True)
    smax = s.abs().amax(-1, keepdim=True)
    ds = (66 * U / 8 * (q.abs() @ k.abs().mT)).amax(-1, keepdim=True) \
        + 8 * U * smax
    o64 = P @ v
    e_o = (RB + 2 * ds + (2 * T + 8) * U) * (P @ v.abs())
    e_lse = ds + (T + 4) * U + 2 * U * (math.log(L) + smax + lse64.abs())

    eP = ds + e_lse + 2 * U * lse64.abs() + 2 * U
    dP = do @ v.mT
    e_dP = 66 * U * (do.abs() @ v.abs().mT)
    delta = (do * o64).sum(-1, keepdim=True)
    e_delta = ((do.abs() * (_hulp(o64.abs() + 1.01 * e_o) + 1.01 * e_o))
               .sum(-1, keepdim=True)
               + 18 * U * (do * o64).abs().sum(-1, keepdim=True))
    dS = P * (dP - delta)
    e_dS = P * (e_dP + e_delta + U * (dP.abs() + delta.abs())) \
        + dS.abs() * (eP + U)
    r_dS = RB * (dS.abs() + e_dS)
    e_dq = ((e_dS + r_dS) @ k.abs() + T * U * (dS.abs() @ k.abs())) / 8
    e_dk = ((e_dS + r_dS).mT @ q.abs() + T * U * (dS.abs().mT @ q.abs())) / 8
    e_dv = ((RB + eP) * P).mT @ do.abs() + T * U * (P.mT @ do.abs())

    qkv = torch.cat([_grid(t, H, W) for t in (q, k, v)], 1).contiguous(
        memory_format=CL)
    dod = _grid(do, H, W)
    if dtype is None:
        o, lse = ext.attn_fwd(qkv, h, True)
        o0, lse0 = ext.attn_fwd(qkv, h, False)
        assert torch.equal(o0, o) and lse0.numel() == 0
        assert lse.shape == (N, h, L) and lse.dtype == torch.float32
        assert bool(((lse.cpu().to(F64)[..., None] - lse64).abs()
                     <= 1.01 * e_lse).all())
        dqkv = ext.attn_bwd(qkv, o, lse, dod, h)
        assert torch.equal(dqkv, ext.attn_bwd(qkv, o, lse, dod, h))
        dtype = BF
    else:
        x = qkv.to(dtype).requires_grad_(True)
        o = F_ops.attention2d(x, h)
        o.backward(dod)
        dqkv = x.grad
    assert o.dtype == BF and o.shape == (N, 64 * h, H, W)
    assert dqkv.dtype == dtype and dqkv.shape == qkv.shape
    assert o.is_contiguous(memory_format=CL)
    assert dqkv.is_contiguous(memory_format=CL)
    _within(_heads(o, h), o64, e_o)
    dq, dk, dv = (_heads(t, h) for t in dqkv.chunk(3, 1))
    _within(dq, dS @ k / 8, e_dq)
    _within(dk, dS.mT @ q / 8, e_dk)
    _within(dv, P.mT @ do, e_dv)
    return _heads(o, h), dv


def _random(N, h, L, seed):
    """q with deviation 4 (logits with deviation 4); every odd row's largest
    logit is moved to one of the last four keys, i.e. into the last tile."""
    g = torch.Generator().manual_seed(seed)
    q = 4 * torch.randn(N, h, L, 64, generator=g, dtype=F64)
    k, v, do = (torch.randn(N, h, L, 64, generator=g, dtype=F64)
                for _ in range(3))
    i = torch.arange(1, L, 2)
    q[:, :, i] += 3 * k[:, :, L - 1 - (i // 2) % min(4, L)]
    return _bf(q), _bf(k), _bf(v), _bf(do)


# the last case has more blocks than the device has CUs: several blocks share
# a CU and a wave's DMA is slow enough to lose a race with the barrier
@pytest.mark.parametrize("N,heads,H,W", CASES + [(32, 3, 14, 14)])
def test_random_data_within_rounding_bounds(N, heads, H, W):
    _check(*_random(N, heads, H * W, 7 * H + W + heads), H, W)


@pytest.mark.parametrize("N,heads,H,W", CASES)
def test_uniform_attention_is_the_exact_mean(N, heads, H, W):
    L = H * W
    g = torch.Generator().manual_seed(L + heads)
    q = torch.zeros(N, heads, L, 64, dtype=F64)
    k = _bf(torch.randn(N, heads, L, 64, generator=g, dtype=F64))
    v = torch.randint(-4, 5, (N, heads, L, 64), generator=g).to(F64)
    qkv = torch.cat([_grid(t, H, W) for t in (q, k, v)], 1).contiguous(
        memory_format=CL)
    o, lse = ext.attn_fwd(qkv, heads, True)
    want = v.sum(2, keepdim=True).expand_as(v) / L
    _within(_heads(o, heads), want, 2 * U * want.abs())
    assert bool(((lse.cpu().to(F64) - math.log(L)).abs()
                 <= 2 * U * math.log(L) + U).all())


@pytest.mark.parametrize("N,heads,H,W", CASES)
def test_one_hot_attention_copies_the_target_row(N, heads, H, W):
    L = H * W
    g = torch.Generator().manual_seed(3 * L + heads)
    j = torch.arange(L)
    code = torch.zeros(L, 64, dtype=F64)
    code[j, j % 14] = 16
    code[j, 14 + j // 14] = 16
    t = (7 * j + 3) % L
    k = code.expand(N, heads, L, 64).clone()
    q = code[t].expand(N, heads, L, 64).clone()
    v = _bf((0.5 + torch.rand(N, heads, L, 64, generator=g, dtype=F64))
            * (2 * torch.randint(0, 2, (N, heads, L, 64), generator=g) - 1))
    do = torch.randint(-4, 5, (N, heads, L, 64), generator=g).to(F64)
    o, dv = _check(q, k, v, do, H, W)
    assert torch.equal(o, v[:, :, t])
    want = torch.zeros_like(do).index_add_(2, t, do)
    wabs = torch.zeros_like(do).index_add_(2, t, do.abs())
    assert torch.equal(dv[want != 0], want[want != 0])
    assert bool(((dv - want).abs() <= 67 * (-(-L // 64)) * U * wabs
                 + 4 * L * math.exp(-32)).all())


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_autograd_returns_the_inputs_dtype(dtype):
    N, heads, H, W = 2, 3, 5, 13
    _check(*_random(N, heads, H * W, 11), H, W, dtype=getattr(torch, dtype))


@pytest.mark.parametrize("shape,heads", [((2, 3 * 32 * 2, 4, 4), 2),
                                         ((2, 192, 16), 1)])
def test_out_of_scope_inputs_raise(shape, heads):
    with pytest.raises(ValueError, match=r"head dimension 64 exactly"):
        F_ops.attention2d(torch.zeros(shape, device=DEV), heads)


def test_vit_tiny_trains_under_amp_with_fused_adamw():
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    x, t = x.to(DEV), torch.arange(4, device=DEV)
    losses = []
    try:
        amp._state.__init__()
        F_ops.clear_weight_cache()
        same_seeds(0)
        model = build_model("vit_tiny", num_classes=10,
                            cifar_stem=True).to(DEV).train()
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        model, opt = amp.initialize(model, opt, opt_level="O1")
        for step in range(20):
            opt.zero_grad()
            loss = F_ops.cross_entropy_loss(model(x), t) / 4
            with amp.scale_loss(loss, opt) as scaled:
                scaled.backward()
            if step == 0:
                for name, p in model.named_parameters():
                    assert p.grad is not None, name
                    assert bool(p.grad.isfinite().all()), name
                assert model.blocks[5].attn.qkv.weight.grad.abs().max() > 0
            opt.step()
            losses.append(loss.detach())
    finally:
        amp._state.__init__()
    losses = torch.stack(losses).cpu()
    assert bool(losses.isfinite().all()) and losses[-1] < losses[0]
