"""FusedAdamW and FusedLAMB on the CPU tier: the torch path against a
float64 hand implementation, the state layout (torch's names, transplants
to and from torch.optim.AdamW), the parameter-group split, the optimizers
under this project's DDP + amp + Lookahead stack over gloo, and the
trainer flags."""
import copy
import os
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_tricks_amd import amp

U = 2.0 ** -24      # fp32 unit roundoff
WORLD = 2
SHAPES = [(7, 5), (33,), (3, 4, 2, 2), (1,), (64, 9)]


# ------------------------------------------------- float64 hand reference ---

def _ref_moments(g, m, v, b1, b2):
    """float64 moments and M >= |m_new|, the same chain on absolute
    values."""
    return (b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g,
            b1 * m.abs() + (1 - b1) * g.abs())


def _state_of(opt, ps):
    return ([p.detach().double().clone() for p in ps],
            [opt.state[p]["exp_avg"].double().clone() if p in opt.state
             else torch.zeros_like(p, dtype=torch.float64) for p in ps],
            [opt.state[p]["exp_avg_sq"].double().clone() if p in opt.state
             else torch.zeros_like(p, dtype=torch.float64) for p in ps])


def _make(seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _grads(ps, seed, zero=None):
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(p.shape, generator=g) * 3.0 for p in ps]
    if zero is not None:
        out[zero].zero_()
    return out


@pytest.mark.parametrize("decoupled", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_adamw_cpu_path_equals_float64_formula(wd, decoupled):
    """Three steps, each against float64 from the state before it; the
    second step has a zero gradient tensor.  The CPU path is fp32 torch
    ops; a Python scalar operand is rounded to fp32 (U) and every op
    rounds once (U = 2**-24).  First-order:

    m.mul_(b1).add_(g, alpha=1-b1): 2U*b1|m| + 2U*(1-b1)|g| + U*M <= 3U*M
    v.mul_(b2).addcmul_(g, g, value=1-b2): 2U*b2*v + 3U*(1-b2)*g*g + U*V,
    all terms non-negative: relative 4U
    d = (v.sqrt() / sqrt(bc2)).add_(eps): 2U + U, constant and division 3U
    (a division by a scalar may be a product with its rounded reciprocal),
    eps and the sum 1U: relative 7U
    p.mul_(1 - lr*wd): 2U*|p|
    p.addcdiv_(m, d, value=-lr/bc1): m/d carries (3U*M + 7U*|m|)/d + U,
    the value and the product 2U, so with R = (lr/bc1)*M/d the update
    carries 13U*R and the sum U*(|p| + R):    U*(3|p| + 14R)
    asserted as U*(4|p| + 15R), the moments as 4U*M and 5U*v.

    decoupled=False, wd != 0: g' = g.add(p, alpha=wd) carries 3U*G with
    G = |g| + wd|p| (constant, product, sum), and p is not decayed.  With
    Mc = b1|m| + (1-b1)*G and Vc = b2*v + (1-b2)*G*G (>= M, V):
    m: 3U*Mc + (1-b1)*3U*G <= 6U*Mc;  v: 4U*V + (1-b2)*2|g'|*3U*G
    <= 10U*Vc, relative ev = 10U*Vc/v_ref, a condition number of the
    reference (large only where g + wd*p cancels);  d: ev/2 + 5U;
    m/d: (6U + ev/2 + 5U + U)*Mc/d, value and product 2U, the sum
    U*(|p| + Rc) with Rc = (lr/bc1)*Mc/d:
        U*|p| + U*(15 + 5*Vc/v_ref)*Rc
    asserted as U*(2|p| + (16 + 6*Vc/v_ref)*Rc), 7U*Mc and 11U*Vc."""
    from ddp_tricks_amd.ops.optim import FusedAdamW
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    ps = _make()
    opt = FusedAdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd,
                     decoupled=decoupled)
    coupled = (not decoupled) and wd != 0
    for step in (1, 2, 3):
        grads = _grads(ps, 10 + step, zero=1 if step == 2 else None)
        p0, m0, v0 = _state_of(opt, ps)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        c0 = lr / bc1
        for i, p in enumerate(ps):
            g = grads[i].double()
            got_m = opt.state[p]["exp_avg"].double()
            got_v = opt.state[p]["exp_avg_sq"].double()
            if coupled:
                G = g.abs() + wd * p0[i].abs()
                m_ref, v_ref, _ = _ref_moments(g + wd * p0[i], m0[i], v0[i],
                                               b1, b2)
                Mc = b1 * m0[i].abs() + (1 - b1) * G
                Vc = b2 * v0[i] + (1 - b2) * G * G
                d = v_ref.sqrt() / bc2 ** 0.5 + eps
                p_ref = p0[i] - c0 * m_ref / d
                cond = torch.where(v_ref > 0, Vc / v_ref,
                                   torch.ones_like(Vc))
                bound = U * (2 * p0[i].abs()
                             + (16 + 6 * cond) * c0 * Mc / d)
                m_bound, v_bound = 7 * U * Mc, 11 * U * Vc
            else:
                m_ref, v_ref, M = _ref_moments(g, m0[i], v0[i], b1, b2)
                d = v_ref.sqrt() / bc2 ** 0.5 + eps
                dec = (1 - lr * wd) if decoupled else 1.0
                p_ref = p0[i] * dec - c0 * m_ref / d
                bound = U * (4 * p0[i].abs() + 15 * c0 * M / d)
                m_bound, v_bound = 4 * U * M, 5 * U * v_ref
            assert bool(((got_m - m_ref).abs() <= m_bound).all()), (step, i)
            assert bool(((got_v - v_ref).abs() <= v_bound).all()), (step, i)
            assert bool(((p.detach().double() - p_ref).abs()
                         <= bound).all()), (step, i)
            assert float(opt.state[p]["step"]) == step
            assert not torch.equal(p.detach().double(), p0[i])
    assert opt._steps.tolist() == [3.0] * len(ps)


@pytest.mark.parametrize("trust_clip", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_lamb_cpu_path_equals_float64_formula(wd, trust_clip):
    """The moments as above.  u = (m / bc1).div_((v / bc2).sqrt_().add_(eps))
    [+ wd*p]: m/bc1 carries 3U*M/bc1 + 3U (constant, possibly a reciprocal
    product), the denominator 4U + 3U, half of it after the root plus its
    own rounding, 4.5U + U, eps and the sum 1U: 7U; the quotient 1U:
    <= 14U*Q with Q = (M/bc1)/d; wd*p adds 2U*wd|p| and the sum
    U*(Q + wd|p|):  |u - u_ref| <= 15U*A, A = Q + wd|p|.
    Both norms are taken in float64, so the ratio's only errors are u's
    (15U*kappa relative, kappa = |A|/|u_ref| from the reference) and its
    own rounding to fp32: RHO = U*(1 + 15*kappa).  p.add_(u, alpha=-lr*r):
    alpha rounds once more,
        |p - p_ref| <= (RHO + U)*lr*r*|u_ref| + lr*r*15U*A + U*(|p| + lr*r*A)
    asserted as (RHO + 2U)*lr*r*|u_ref| + U*(2|p| + 17*lr*r*A)."""
    from ddp_tricks_amd.ops.optim import FusedLAMB
    lr, b1, b2, eps, max_trust = 1e-2, 0.9, 0.999, 1e-6, 1.2
    ps = _make()
    opt = FusedLAMB(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd,
                    trust_clip=trust_clip, max_trust=max_trust)
    clipped = 0
    for step in (1, 2, 3):
        grads = _grads(ps, 10 + step, zero=1 if step == 2 else None)
        p0, m0, v0 = _state_of(opt, ps)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        assert opt.trust_ratios.dtype == torch.float32
        assert opt.trust_ratios.shape == (len(ps),)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        for i, p in enumerate(ps):
            g = grads[i].double()
            m_ref, v_ref, M = _ref_moments(g, m0[i], v0[i], b1, b2)
            d = (v_ref / bc2).sqrt() + eps
            u_ref = (m_ref / bc1) / d + wd * p0[i]
            A = (M / bc1) / d + wd * p0[i].abs()
            wn, un = float(p0[i].norm()), float(u_ref.norm())
            r = wn / un
            rho = U * (1 + 15 * float(A.norm()) / un)
            want = min(r, max_trust) if trust_clip else r
            clipped += int(trust_clip and r > max_trust)
            assert abs(float(opt.trust_ratios[i]) - want) <= rho * r, i
            rr = want * (1 + rho)
            p_ref = p0[i] - lr * want * u_ref
            bound = ((rho + 2 * U) * lr * rr * u_ref.abs()
                     + U * (2 * p0[i].abs() + 17 * lr * rr * A))
            assert bool(((p.detach().double() - p_ref).abs()
                         <= bound).all()), (step, i)
    assert clipped > 0 or not trust_clip


def test_lamb_degenerate_mixed_groups_and_missing_gradients():
    """Zero-norm tensors get ratio 1; adapt=False groups take exactly the
    FusedAdamW step; a parameter without a gradient keeps its value, its
    step and its ratio; zero_grad keeps the storage."""
    from ddp_tricks_amd.ops.optim import FusedAdamW, FusedLAMB

    def make():
        gen = torch.Generator().manual_seed(7)
        a = [torch.nn.Parameter(torch.randn(6, 3, generator=gen)),
             torch.nn.Parameter(torch.zeros(5, 2)),
             torch.nn.Parameter(torch.randn(4, 4, generator=gen))]
        b = [torch.nn.Parameter(torch.randn(9, generator=gen)),
             torch.nn.Parameter(torch.randn(3, generator=gen))]
        return a, b
    a, b = make()
    _, b2 = make()
    g = torch.Generator().manual_seed(6)
    grads = [torch.randn(p.shape, generator=g) for p in a + b]
    grads[2].zero_()
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-7)
    lamb = FusedLAMB([dict(params=a, weight_decay=0.0),
                      dict(params=b, adapt=False, weight_decay=0.02)], **kw)
    adamw = FusedAdamW(b2, weight_decay=0.02, **kw)
    for p, gr in zip(a + b, grads):
        p.grad = gr.clone()
    for p, gr in zip(b2, grads[3:]):
        p.grad = gr.clone()
    a2_before = a[2].detach().clone()
    for step in range(2):
        lamb.step()
        adamw.step()
        ratios = lamb.trust_ratios
        # a[1] was all zero before the first step only; a[2] has zero
        # gradients and moments throughout, so u = 0 there (wd = 0)
        assert ratios.tolist()[2:] == [1.0, 1.0, 1.0]
        assert (float(ratios[1]) == 1.0) == (step == 0)
        assert float(ratios[0]) > 0.0
    assert lamb.trust_ratios is ratios                       # reused
    assert torch.equal(a[2].detach(), a2_before)
    for p, q in zip(b, b2):
        assert torch.equal(p.detach(), q.detach())
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(lamb.state[p][key], adamw.state[q][key])
    assert all(bool(torch.isfinite(p).all()) for p in a + b)
    assert lamb._steps.tolist() == [2.0] * 5
    before = [p.detach().clone() for p in a]
    r1 = float(lamb.trust_ratios[1])
    a[1].grad = None
    a[2].grad = torch.ones(4, 4)
    lamb.step()
    assert torch.equal(a[1].detach(), before[1])
    assert float(lamb.trust_ratios[1]) == r1
    assert not torch.equal(a[0].detach(), before[0])
    assert not torch.equal(a[2].detach(), before[2])
    assert lamb._steps.tolist() == [3.0, 2.0, 3.0, 3.0, 3.0]
    assert float(lamb.state[a[1]]["step"]) == 2.0
    ptr = a[0].grad.data_ptr()
    lamb.zero_grad()
    assert a[0].grad.data_ptr() == ptr and not bool(a[0].grad.any())


def test_constructor_validation_and_exports():
    from ddp_tricks_amd import ops
    from ddp_tricks_amd.ops.optim import FusedAdamW, FusedLAMB
    assert ops.FusedAdamW is FusedAdamW and ops.FusedLAMB is FusedLAMB
    p = [torch.nn.Parameter(torch.ones(2, 2))]
    for cls in (FusedAdamW, FusedLAMB):
        with pytest.raises(ValueError):
            cls(p, lr=-1.0)
        with pytest.raises(ValueError):
            cls(p, lr=1e-3, betas=(1.0, 0.999))
        with pytest.raises(ValueError):
            cls(p, lr=1e-3, eps=-1.0)
        with pytest.raises(ValueError):
            cls(p, lr=1e-3, weight_decay=-0.1)
    with pytest.raises(ValueError):
        FusedLAMB(p, lr=1e-3, max_trust=0.0)
    grp = FusedAdamW(p, lr=1e-3).param_groups[0]
    assert (grp["betas"], grp["eps"], grp["weight_decay"],
            grp["decoupled"]) == ((0.9, 0.999), 1e-8, 0.01, True)
    grp = FusedLAMB(p, lr=1e-3).param_groups[0]
    assert (grp["adapt"], grp["trust_clip"], grp["max_trust"]) == (
        True, False, 10.0)


# ------------------------------------------------------------ state layout ---

def _pair_bound(p, g, m, v, lr, b1, b2, eps, step):
    """|ours - torch.optim.AdamW| after one step from the same fp32 state.
    Ours is within U*(3|p| + 14R) of float64 (see above).  torch differs in
    one place, m.lerp_(g, 1-b1) = m + w*(g - m): the difference rounds
    (U*(|g| + |m|)), w and the product round (2U), the sum rounds:
        |m_t - m_ref| <= U*Mt,  Mt = |m| + 4*(1-b1)*(|g| + |m|)
    and the rest of its chain is ours, so it is within
    U*(3|p| + c0*Mt/d + 11R).  The sum, with the usual one-up:
        U*(8|p| + 27R + 2*c0*Mt/d)."""
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    c0 = lr / bc1
    _, v_ref, M = _ref_moments(g, m, v, b1, b2)
    d = v_ref.sqrt() / bc2 ** 0.5 + eps
    Mt = m.abs() + 4 * (1 - b1) * (g.abs() + m.abs())
    return U * (8 * p.abs() + 27 * c0 * M / d + 2 * c0 * Mt / d)


@pytest.mark.parametrize("direction", ["to_torch", "from_torch"])
def test_state_transplants_with_torch_adamw(direction):
    from ddp_tricks_amd.ops.optim import FusedAdamW
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 0.05
    ours_p, torch_p = _make(), _make()
    ours = FusedAdamW(ours_p, lr=lr, betas=(b1, b2), eps=eps,
                      weight_decay=wd)
    ref = torch.optim.AdamW(torch_p, lr=lr, betas=(b1, b2), eps=eps,
                            weight_decay=wd, foreach=False)
    src, src_p = (ours, ours_p) if direction == "to_torch" else (ref, torch_p)
    dst, dst_p = (ref, torch_p) if direction == "to_torch" else (ours, ours_p)
    for step in (1, 2, 3):
        for p, g in zip(src_p, _grads(src_p, 20 + step)):
            p.grad = g
        src.step()
    # a copy, as out of a checkpoint file: load_state_dict keeps the
    # tensors it is given, and the two optimizers must not share moments
    sd = copy.deepcopy(src.state_dict())
    for st in sd["state"].values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dim() == 0 and st["step"].dtype == torch.float32
        assert float(st["step"]) == 3.0
        assert st["step"].untyped_storage().nbytes() == 4
    dst.load_state_dict({"state": sd["state"],
                         "param_groups": dst.state_dict()["param_groups"]})
    with torch.no_grad():
        for a, b in zip(dst_p, src_p):
            a.copy_(b)
    assert ours._steps.tolist() == [3.0] * len(SHAPES)
    assert all(float(ours.state[p]["step"]) == 3.0 for p in ours_p)
    p0, m0, v0 = _state_of(ours, ours_p)
    grads = _grads(ours_p, 29)
    for p, q, g in zip(ours_p, torch_p, grads):
        p.grad, q.grad = g.clone(), g.clone()
    ours.step()
    ref.step()
    for i, (p, q) in enumerate(zip(ours_p, torch_p)):
        assert float(ours.state[p]["step"]) == 4.0
        assert float(ref.state[q]["step"]) == 4.0
        bound = _pair_bound(p0[i], grads[i].double(), m0[i], v0[i], lr, b1,
                            b2, eps, 4)
        diff = (p.detach().double() - q.detach().double()).abs()
        assert bool((diff <= bound).all()), i
        assert not torch.equal(p.detach().double(), p0[i])
    assert ours._steps.tolist() == [4.0] * len(SHAPES)


def test_state_dict_round_trip_keeps_the_counter():
    """state_dict -> a fresh optimizer -> the next steps are bitwise those
    of the original; parameters that never stepped stay at step 0."""
    from ddp_tricks_amd.ops.optim import FusedLAMB
    a_p, b_p = _make(), _make()
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.05)
    a, b = FusedLAMB(a_p, **kw), FusedLAMB(b_p, **kw)
    for step in (1, 2):
        for i, (p, g) in enumerate(zip(a_p, _grads(a_p, 40 + step))):
            p.grad = None if i == 3 else g
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert 3 not in sd["state"]
    b.load_state_dict(sd)
    with torch.no_grad():
        for p, q in zip(a_p, b_p):
            q.copy_(p)
    assert b._steps.tolist() == [2.0, 2.0, 2.0, 0.0, 2.0]
    for p, q, g in zip(a_p, b_p, _grads(a_p, 49)):
        p.grad, q.grad = g.clone(), g.clone()
    a.step()
    b.step()
    assert b._steps.tolist() == [3.0, 3.0, 3.0, 1.0, 3.0]
    for p, q in zip(a_p, b_p):
        assert torch.equal(p.detach(), q.detach())
    assert torch.equal(a.trust_ratios, b.trust_ratios)


@pytest.mark.parametrize("name", ["toy_net", "resnet18"])
def test_decay_param_groups_split(name):
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import decay_param_groups
    model = build_model(name)
    groups = decay_param_groups(model, 0.05)
    assert len(groups) == 2
    decayed, plain = groups
    assert decayed["adapt"] is True and decayed["weight_decay"] == 0.05
    assert plain["adapt"] is False and plain["weight_decay"] == 0.0
    assert decayed["params"] and plain["params"]
    assert all(p.ndim > 1 for p in decayed["params"])
    assert all(p.ndim <= 1 for p in plain["params"])
    got = [id(p) for g in groups for p in g["params"]]
    want = [id(p) for p in model.parameters()]
    assert len(got) == len(set(got)) == len(want)
    assert set(got) == set(want)
    plain_ids = {id(p) for p in plain["params"]}
    for n, p in model.named_parameters():
        if n.endswith(".bias") or "bn" in n.split(".")[-2]:
            assert id(p) in plain_ids, n


def test_clip_fused_recognises_the_new_classes(monkeypatch):
    from ddp_tricks_amd.ops.optim import FusedAdamW, FusedLAMB
    from ddp_tricks_amd.utils.lookahead import Lookahead
    monkeypatch.delenv("DDPX_CLIP_FUSED", raising=False)
    p = [torch.nn.Parameter(torch.ones(2, 2))]
    for cls in (FusedAdamW, FusedLAMB):
        opt = cls(p, lr=1e-3)
        assert amp._clip_fused(opt) and amp._clip_fused(Lookahead(opt))
    assert not amp._clip_fused(torch.optim.AdamW(p, lr=1e-3))
    monkeypatch.setenv("DDPX_CLIP_FUSED", "0")
    assert not amp._clip_fused(FusedAdamW(p, lr=1e-3))


# ------------------------------------------------------- world-2 full stack ---

class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from ddp_tricks_amd.ops.modules import (BatchNorm1d, BatchNorm2d,
                                                Conv2d, Linear)
        self.conv = Conv2d(1, 4, 3, padding=1)
        self.bn = BatchNorm2d(4, fuse_relu=True)
        self.fc = Linear(4 * 4 * 4, 8)
        self.bn1 = BatchNorm1d(8)
        self.head = Linear(8, 3)

    def forward(self, x):
        x = self.bn(self.conv(x))
        return self.head(torch.relu(self.bn1(self.fc(x.flatten(1)))))


def _worker_stack(rank, port, name, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from ddp_tricks_amd import ops
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    from ddp_tricks_amd.utils.lookahead import Lookahead
    amp._state.__init__()
    torch.manual_seed(7)
    model = _Net()
    cls = {"adamw": ops.FusedAdamW, "lamb": ops.FusedLAMB}[name]
    opt = cls(ops.decay_param_groups(model, 0.05), lr=1e-2,
              betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    la = Lookahead(opt, k=2, alpha=0.5)
    model, apex_opt = amp.initialize(model, la, "O1", max_grad_norm=1.0)
    ddp = DDP(model)
    torch.manual_seed(500 + rank)             # DIFFERENT data per rank
    sigs = []
    for step in range(4):
        apex_opt.zero_grad(set_to_none=(step == 2))
        x = torch.randn(4, 1, 4, 4)
        t = torch.randn(4, 3)
        ddp.train()
        loss = ((ddp(x) - t) ** 2).mean()
        with amp.scale_loss(loss, apex_opt) as sl:
            sl.backward()
        apex_opt.step()
        ratios = getattr(opt, "trust_ratios", None)
        sigs.append(([p.detach().numpy().tobytes()
                      for p in model.parameters()],
                     opt._steps.tolist(),
                     None if ratios is None else ratios.tolist()))
    n_decayed = len(opt.param_groups[0]["params"])
    amp._state.__init__()
    results.put((rank, (sigs, n_decayed)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("name,port", [("adamw", 29646), ("lamb", 29647)])
def test_world2_full_stack_in_bitwise_lockstep(name, port):
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=_worker_stack, args=(r, port, name, results))
             for r in range(WORLD)]
    [p.start() for p in procs]
    got = dict(results.get(timeout=110) for _ in range(WORLD))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    (s0, n_decayed), (s1, _) = got[0], got[1]
    for step in range(4):
        assert s0[step][0] == s1[step][0], f"params differ at step {step}"
        assert s0[step][1] == s1[step][1] == [step + 1.0] * 10
        assert s0[step][2] == s1[step][2], f"ratios differ at step {step}"
        if name == "lamb":
            ratios = s0[step][2]
            assert all(0.0 < r < float("inf") for r in ratios[:n_decayed])
            assert ratios[n_decayed:] == [1.0] * (10 - n_decayed)
    assert n_decayed == 3
    assert s0[0][0] != s0[3][0]                              # it trained


# ------------------------------------------------------------- trainer flags ---

def _load_run():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_adamw", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_flags(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    a = run.parse_args()
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == (
        "sgd", 0.9, 0.999, 1e-8)
    assert a.learning_rate == 1e-1                   # -l keeps its default
    for name in ("adamw", "lamb"):
        monkeypatch.setattr(sys, "argv", [
            "run.py", "--optimizer", name, "-l", "1e-3", "--weight_decay",
            "0.05", "--adam_beta1", "0.8", "--adam_beta2", "0.95",
            "--adam_eps", "1e-6", "--resume"])
        a = run.parse_args()
        assert (a.optimizer, a.learning_rate, a.weight_decay) == (
            name, 1e-3, 0.05)
        assert (a.adam_beta1, a.adam_beta2, a.adam_eps) == (0.8, 0.95, 1e-6)
        assert a.resume is True
    monkeypatch.setattr(sys, "argv", ["run.py", "--optimizer", "adam"])
    with pytest.raises(SystemExit):
        run.parse_args()


def _args(tmp_path, name, epochs, **over):
    a = types.SimpleNamespace(
        exp_name=name, learning_rate=0.05, batch_size=64, epochs=epochs,
        warmup_epochs=2, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.fixture
def dist_env():
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29648")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("gloo", rank=0, world_size=1)
    yield


class _Stop(Exception):
    pass


def _built_optimizer(tmp_path, monkeypatch, **over):
    """The optimizer train() hands to Lookahead (training is cut there)."""
    import importlib
    train_mod = importlib.import_module("ddp_tricks_amd.utils.train")
    seen = []

    def spy(optimizer, **kw):
        seen.append((optimizer, kw))
        raise _Stop

    monkeypatch.setattr(train_mod, "Lookahead", spy)
    amp._state.__init__()
    with pytest.raises(_Stop):
        train_mod.train(_args(tmp_path, "BUILD", 1, **over))
    amp._state.__init__()
    return seen[0]


def test_default_flags_still_build_fused_sgd(tmp_path, monkeypatch, dist_env):
    from ddp_tricks_amd.ops.optim import FusedSGD
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    for over in ({}, dict(adam_beta1=0.5, adam_beta2=0.6, adam_eps=1.0)):
        opt, kw = _built_optimizer(tmp_path, monkeypatch, **over)
        assert type(opt) is FusedSGD and kw == dict(k=10, alpha=0.5)
        assert len(opt.param_groups) == 1
        grp = opt.param_groups[0]
        assert set(grp) >= {"lr", "momentum", "weight_decay", "nesterov"}
        assert "betas" not in grp and "adapt" not in grp
        assert (grp["lr"], grp["momentum"], grp["nesterov"],
                grp["weight_decay"]) == (0.05, 0.9, True, 0)


@pytest.mark.parametrize("name", ["adamw", "lamb"])
def test_adam_flags_build_the_fused_optimizer(name, tmp_path, monkeypatch,
                                              dist_env):
    from ddp_tricks_amd.ops.optim import FusedAdamW, FusedLAMB
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    opt, kw = _built_optimizer(
        tmp_path, monkeypatch, optimizer=name, learning_rate=1e-3,
        weight_decay=0.05, adam_beta1=0.8, adam_beta2=0.95, adam_eps=1e-6)
    assert type(opt) is (FusedAdamW if name == "adamw" else FusedLAMB)
    assert kw == dict(k=10, alpha=0.5)
    decayed, plain = opt.param_groups
    assert decayed["weight_decay"] == 0.05 and plain["weight_decay"] == 0.0
    assert decayed["adapt"] is True and plain["adapt"] is False
    assert all(p.ndim > 1 for p in decayed["params"])
    assert all(p.ndim <= 1 for p in plain["params"])
    for grp in opt.param_groups:
        assert (grp["lr"], grp["betas"], grp["eps"]) == (
            1e-3, (0.8, 0.95), 1e-6)
    if name == "adamw":
        assert decayed["decoupled"] is True
    # the flags' defaults when a caller's namespace lacks them
    opt, _ = _built_optimizer(tmp_path, monkeypatch, optimizer=name,
                              learning_rate=1e-3)
    assert (opt.param_groups[0]["betas"], opt.param_groups[0]["eps"]) == (
        (0.9, 0.999), 1e-8)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["adamw", "lamb"])
def test_resume_bitwise_equals_straight_run(name, tmp_path, monkeypatch,
                                            dist_env):
    """`run.py --optimizer NAME --weight_decay 0.05 --resume`: 2 epochs +
    resume for 1 more equals 3 straight epochs, bit for bit: moments, step
    counters and Lookahead's slow weights all come back."""
    from ddp_tricks_amd.utils.train import train
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "256")
    flags = dict(resume=True, optimizer=name, weight_decay=0.05,
                 learning_rate=2e-3)

    amp._state.__init__()
    train(_args(tmp_path, "STRAIGHT", 3, **flags))
    ck = torch.load(os.path.join(tmp_path, "STRAIGHT.resume.pt"),
                    weights_only=False)
    straight = ck["model"]
    groups = ck["optimizer"]["param_groups"]
    assert [g["adapt"] for g in groups] == [True, False]
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0]
    fast = ck["optimizer"]["fast_state"]
    assert len(fast) == sum(len(g["params"]) for g in groups)
    counts = set()
    for st in fast.values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dim() == 0 and st["step"].dtype == torch.float32
        counts.add(float(st["step"]))
    assert counts == {12.0}                          # 3 epochs x 4 batches

    amp._state.__init__()
    train(_args(tmp_path, "SPLIT", 2, **flags))
    amp._state.__init__()
    train(_args(tmp_path, "SPLIT", 3, **flags))
    amp._state.__init__()
    split = torch.load(os.path.join(tmp_path, "SPLIT.resume.pt"),
                       weights_only=False)
    for k in straight:
        assert torch.equal(straight[k], split["model"][k]), k
        assert bool(torch.isfinite(straight[k]).all()), k
    for k, st in split["optimizer"]["fast_state"].items():
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(st[key], fast[k][key]), (k, key)
