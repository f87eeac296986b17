"""Invalidation of the per-parameter bf16 operand cache (weight_variant).

The cache keys its entries on ``Tensor._version``.  Every write the
autograd version counter sees must invalidate all five variants, and every
writer that goes AROUND the counter (through ``p.data`` or a raw pointer:
FusedSGD, Lookahead, the DDP parameter broadcast) must leave no stale
entry behind.  A stale entry is silent: the next forward and dgrad simply
compute with the old weights.

CPU tier: each variant after each kind of write is compared with a bf16
transform built here from the new weights (``_fresh`` — written
independently of weight_variant).  GPU tier (@pytest.mark.gpu): integer
weights and gradients, lr = 0.5, so the updated weights are half-integers
that bf16 holds exactly; conv / linear forward and backward through the
public entry points must equal the float64 result for the UPDATED weights
(``torch.equal``; the 2^24 bound of test_gpu_exact.py, taken in units of
the terms' common denominator 1/2, is asserted on the reference alone).
"""
import os
import zlib

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops.functional import clear_weight_cache, weight_variant
from ddp_tricks_amd.ops.optim import FusedSGD
from ddp_tricks_amd.utils.lookahead import Lookahead

BF = torch.bfloat16
CL = torch.channels_last
VARIANTS = ["flat", "nhwc", "wt2", "nhwc_p8", "wt2_p8"]
WSHAPE = (4, 3, 2, 2)        # K, C, R, S with C < 8 so the _p8 variants pad


def _fresh(w, variant):
    """bf16 transform of the CURRENT values of w, built from scratch."""
    wb = w.detach().clone().to(BF)
    if variant == "flat":
        return wb.contiguous()
    K, C, R, S = wb.shape
    if variant.endswith("_p8"):
        wp = torch.zeros(K, 8, R, S, dtype=BF, device=wb.device)
        wp[:, :C] = wb
        wb, C = wp, 8
    if variant.startswith("nhwc"):
        return wb.contiguous(memory_format=CL)
    # wt2[c, (r*S + s)*K + k] = w[k, c, r, s]
    return torch.stack([wb[:, c].permute(1, 2, 0).reshape(-1)
                        for c in range(C)])


def _same(got, want):
    return (got.shape == want.shape and got.dtype == want.dtype
            and got.stride() == want.stride() and torch.equal(got, want))


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(autouse=True)
def _empty_cache():
    clear_weight_cache()
    yield
    clear_weight_cache()


# ------------------------------------------------------------- CPU tier ---

def _write_mul(mod):
    with torch.no_grad():
        mod.weight.mul_(-1.75)


def _write_copy(mod):
    with torch.no_grad():
        mod.weight.copy_(_randn(WSHAPE, 2))


def _write_load_state_dict(mod):
    sd = {k: _randn(v.shape, 3 + i)
          for i, (k, v) in enumerate(mod.state_dict().items())}
    mod.load_state_dict(sd)


def _write_sgd(mod):
    opt = torch.optim.SGD(mod.parameters(), lr=0.5)
    mod.weight.grad = _randn(WSHAPE, 5)
    opt.step()


WRITES = {"mul_": _write_mul, "copy_": _write_copy,
          "load_state_dict": _write_load_state_dict, "sgd_step": _write_sgd}


def test_fresh_transform_layouts():
    """_fresh really builds the documented layouts (element by element)."""
    w = _randn(WSHAPE, 0)
    K, C, R, S = WSHAPE
    wb = w.to(BF)
    wt2 = _fresh(w, "wt2_p8")
    assert wt2.shape == (8, R * S * K) and wt2.is_contiguous()
    for k, c, r, s in [(0, 0, 0, 0), (3, 2, 1, 0), (1, 1, 0, 1), (2, 2, 1, 1)]:
        assert wt2[c, (r * S + s) * K + k] == wb[k, c, r, s]
        assert _fresh(w, "wt2")[c, (r * S + s) * K + k] == wb[k, c, r, s]
    assert not wt2[C:].any()
    p8 = _fresh(w, "nhwc_p8")
    assert p8.shape == (K, 8, R, S) and p8.is_contiguous(memory_format=CL)
    assert torch.equal(p8[:, :C], wb) and not p8[:, C:].any()
    assert _fresh(w, "nhwc").is_contiguous(memory_format=CL)


@pytest.mark.parametrize("write", list(WRITES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_follows_versioned_write(variant, write):
    mod = torch.nn.Conv2d(WSHAPE[1], WSHAPE[0], WSHAPE[2], bias=False)
    with torch.no_grad():
        mod.weight.copy_(_randn(WSHAPE, 1))
    w = mod.weight
    old = weight_variant(w, variant)
    assert _same(old, _fresh(w, variant))
    assert weight_variant(w, variant) is old          # a hit is a hit
    old = old.clone()
    WRITES[write](mod)
    assert mod.weight is w
    got = weight_variant(w, variant)
    assert _same(got, _fresh(w, variant))
    assert not torch.equal(got, old)                  # the write was real


@pytest.mark.parametrize("variant", VARIANTS)
def test_data_write_needs_explicit_clear(variant):
    """The documented rule: a write through .data is followed by
    clear_weight_cache(), after which every variant is rebuilt."""
    w = torch.nn.Parameter(_randn(WSHAPE, 1))
    weight_variant(w, variant)
    w.data.mul_(2)
    clear_weight_cache()
    assert _same(weight_variant(w, variant), _fresh(w, variant))
    w.data = _randn(WSHAPE, 9)
    clear_weight_cache()
    assert _same(weight_variant(w, variant), _fresh(w, variant))


def _check_all_variants(params):
    for p in params:
        for v in (VARIANTS if p.dim() == 4 else ["flat"]):
            assert _same(weight_variant(p, v), _fresh(p, v)), (tuple(p.shape), v)


@pytest.mark.parametrize("inner", ["torch_sgd", "fused_sgd"])
def test_lookahead_torch_path_leaves_no_stale_entry(inner):
    """Lookahead.update writes the interpolated slow weights back into the
    fast ones through .data; operands cached since the last fast step must
    not survive it."""
    params = [torch.nn.Parameter(_randn(WSHAPE, 1)),
              torch.nn.Parameter(_randn((5, 6), 2))]
    if inner == "torch_sgd":
        opt = torch.optim.SGD(params, lr=0.5)
    else:
        opt = FusedSGD(params, lr=0.5)
    la = Lookahead(opt, k=2, alpha=0.5)
    seen_change = False
    for step in range(4):
        for i, p in enumerate(params):
            p.grad = _randn(p.shape, 10 * step + i)
        _check_all_variants(params)                   # primes the cache
        la.step()
        _check_all_variants(params)
        # an update on its own (the public update_lookahead) with operands
        # cached after the fast step
        for i, p in enumerate(params):
            with torch.no_grad():
                p.add_(_randn(p.shape, 100 + 10 * step + i))
        _check_all_variants(params)                   # primes the cache
        before = [p.detach().clone() for p in params]
        la.update_lookahead()
        seen_change |= any(not torch.equal(b, p) for b, p in
                           zip(before, params))
        _check_all_variants(params)
    assert seen_change


# ----------------------------------------------------- CPU tier, 2 ranks ---

WORLD = 2


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from ddp_tricks_amd.ops.modules import Conv2d, Linear
        self.conv_small = Conv2d(3, 8, 3, padding=1)      # C < 8: _p8 used
        self.conv = Conv2d(8, 8, 3, padding=1)
        self.fc = Linear(8, 4)


def _net_variants(model):
    """name/variant -> fp32 numpy of weight_variant() for every parameter
    (numpy: tensors over an mp queue race with worker exit)."""
    out = {}
    for name, p in model.named_parameters():
        for v in (VARIANTS if p.dim() == 4 else ["flat"]):
            t = weight_variant(p, v)
            out[f"{name}/{v}"] = (tuple(t.shape), tuple(t.stride()),
                                  t.float().numpy().copy())
    return out


def _worker_ddp_cache(rank, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    torch.manual_seed(100 + rank)                 # DIFFERENT init per rank
    model = _Net()
    pre = _net_variants(model)      # what a forward before the wrap caches
    DDP(model)
    if rank == 1:
        results.put((pre, _net_variants(model)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_ddp_wrap_drops_pre_broadcast_operands():
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    port = 29641
    procs = [ctx.Process(target=_worker_ddp_cache, args=(r, port, results))
             for r in range(WORLD)]
    [p.start() for p in procs]
    pre, post = results.get(timeout=110)
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)

    torch.manual_seed(100)                        # rank 0's init
    ref = _Net()
    differs = False
    for name, p in ref.named_parameters():
        for v in (VARIANTS if p.dim() == 4 else ["flat"]):
            want = _fresh(p, v)
            shape, stride, got = post[f"{name}/{v}"]
            assert shape == tuple(want.shape), (name, v)
            assert stride == tuple(want.stride()), (name, v)
            assert torch.equal(torch.from_numpy(got), want.float()), (name, v)
            differs |= not torch.equal(torch.from_numpy(pre[f"{name}/{v}"][2]),
                                       want.float())
    assert differs            # rank 1 really started from other weights


# ------------------------------------------------------------- GPU tier ---

EXACT_LIMIT = float(2 ** 24)


def _ints(shape, lo, hi, *key):
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, key)).encode()))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _assert_exact_ok(abs_sum, denom):
    """Every term is a multiple of 1/denom: in units of 1/denom the sum of
    |terms| of each output element stays below 2^24."""
    assert (abs_sum.abs().max() * denom).item() < EXACT_LIMIT


def _assert_half_integers(w64):
    """The expected weights are multiples of 1/2 that bf16 holds exactly,
    so each product with an integer activation is a multiple of 1/2."""
    assert torch.equal((w64 * 2).round(), w64 * 2)
    assert torch.equal(w64.to(BF).double(), w64)


def _bf16_round(t64):
    return t64.float().to(BF)


def _steps(params, w0s):
    """Run the update sequence on the device parameters and yield, after
    each phase, the float64 weights the parameters must now hold."""
    opt = FusedSGD(params, lr=0.5, momentum=0.0, weight_decay=0.0)

    def set_grads(tag, mult):
        gs = [_ints(w.shape, -2, 2, tag, i) * mult for i, w in enumerate(w0s)]
        for p, g in zip(params, gs):
            p.grad = g.float().to(p.device)
        return gs

    # phase A: one plain FusedSGD step           w1 = w0 - g1/2
    g1 = set_grads("g1", 1)
    yield "start", [w.clone() for w in w0s]
    opt.step()
    w1 = [w - 0.5 * g for w, g in zip(w0s, g1)]
    yield "fused_sgd", w1
    # phase B: first Lookahead step (slow := fast, interpolation is a no-op)
    la = Lookahead(opt, k=1, alpha=0.5)
    g2 = set_grads("g2", 1)
    la.step()
    w2 = [w - 0.5 * g for w, g in zip(w1, g2)]
    yield "lookahead_init", w2
    # phase C: fast = w2 - g3/2; slow = w2 + (fast - w2)/2; fast := slow.
    # g3 is even so the result stays on the half-integer grid
    g3 = set_grads("g3", 2)
    la.step()
    w3 = [w - 0.25 * g for w, g in zip(w2, g3)]
    yield "lookahead_interp", w3


CONV_CASES = [
    # N, C, H, W, K, R, S, stride, pad
    (2, 8, 5, 7, 8, 3, 3, 1, 1),      # nhwc / wt2
    (2, 3, 9, 7, 16, 3, 3, 1, 1),     # nhwc_p8 fwd, unpadded x saved, wt2_p8
    (1, 3, 32, 32, 8, 3, 3, 1, 1),    # pad8 backward: nhwc_p8 / wt2_p8
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONV_CASES,
                         ids=lambda s: "C%dH%d" % (s[1], s[2]))
def test_gpu_conv_sees_updated_weights_exact(shape):
    dev = torch.device("cuda:0")
    N, C, H, W, K, R, S, stride, pad = shape
    assert F_ops._use_pad8(C, H, W) == (shape == CONV_CASES[2])
    w0 = _ints((K, C, R, S), -1, 1, "w0", shape)
    x = _ints((N, C, H, W), -2, 2, "x", shape)
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    dy = _ints((N, K, P, Q), -2, 2, "dy", shape)
    wp = torch.nn.Parameter(w0.float().to(dev))
    xd = x.to(BF).to(dev).contiguous(memory_format=CL)
    dyd = dy.to(BF).to(dev).contiguous(memory_format=CL)
    phases = []
    for phase, (w,) in _steps([wp], [w0]):
        phases.append(phase)
        _assert_half_integers(w)
        ref_y = F.conv2d(x, w, None, stride, pad)
        ref_dx = torch.nn.grad.conv2d_input((N, C, H, W), w, dy,
                                            stride=stride, padding=pad)
        _assert_exact_ok(F.conv2d(x.abs(), w.abs(), None, stride, pad), 2)
        _assert_exact_ok(torch.nn.grad.conv2d_input(
            (N, C, H, W), w.abs(), dy.abs(), stride=stride, padding=pad), 2)
        assert torch.equal(wp.detach().cpu().double(), w), phase
        xg = xd.clone().requires_grad_(True)
        y = F_ops.conv2d(xg, wp, None, stride, pad)       # fills the cache
        assert torch.equal(y.detach().cpu(), _bf16_round(ref_y)), phase
        (dx,) = torch.autograd.grad(y, xg, dyd)
        assert dx.dtype == BF and dx.shape == (N, C, H, W)
        assert torch.equal(dx.cpu(), _bf16_round(ref_dx)), phase
        # packing-kernel route == torch route of weight_variant (a CPU copy
        # of the parameter takes the latter), every variant
        wc = torch.nn.Parameter(wp.detach().cpu())
        for v in VARIANTS[1:] if C < 8 else ["nhwc", "wt2"]:
            got, want = weight_variant(wp, v), weight_variant(wc, v)
            assert _same(got.cpu(), want), (phase, v)
            assert _same(want, _fresh(wc, v)), (phase, v)
    assert phases == ["start", "fused_sgd", "lookahead_init",
                      "lookahead_interp"]


@pytest.mark.gpu
@pytest.mark.parametrize("mnk", [(5, 10, 24), (5, 17, 24)],
                         ids=["head", "gemm"])
def test_gpu_linear_sees_updated_weights_exact(mnk):
    dev = torch.device("cuda:0")
    M, N, K = mnk
    w0 = _ints((N, K), -1, 1, "lw0", mnk)
    x = _ints((M, K), -2, 2, "lx", mnk)
    dy = _ints((M, N), -2, 2, "ldy", mnk)
    wp = torch.nn.Parameter(w0.float().to(dev))
    xd, dyd = x.to(BF).to(dev), dy.to(BF).to(dev)
    for phase, (w,) in _steps([wp], [w0]):
        _assert_half_integers(w)
        _assert_exact_ok(x.abs() @ w.abs().t(), 2)
        _assert_exact_ok(dy.abs() @ w.abs(), 2)
        assert torch.equal(wp.detach().cpu().double(), w), phase
        xg = xd.clone().requires_grad_(True)
        y = F_ops.linear(xg, wp, None)
        assert torch.equal(y.detach().cpu(), _bf16_round(x @ w.t())), phase
        (dx,) = torch.autograd.grad(y, xg, dyd)
        assert dx.dtype == BF and dx.shape == (M, K)
        assert torch.equal(dx.cpu(), _bf16_round(dy @ w)), phase
        wc = torch.nn.Parameter(wp.detach().cpu())
        assert _same(weight_variant(wp, "flat").cpu(),
                     weight_variant(wc, "flat")), phase
