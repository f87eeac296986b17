"""FusedLARS on the CPU tier: the torch path against a float64 hand
implementation, the parameter-group split, the optimizer under this
project's DDP + amp + Lookahead stack over gloo, and the trainer flags."""
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


# ------------------------------------------------- float64 hand reference ---

def _ref_step(p, g, buf, lr, mu, wd, nesterov, eta, eps, trust_clip,
              adapt=True):
    """One LARS step on float64 copies.  Returns (p, buf, ratio, D, B): D and
    B are the same chains evaluated on absolute values, upper bounds of |d|
    and |buf| used to scale the rounding bound."""
    p, g, buf = p.double(), g.double(), buf.double()
    wn, gn = float(p.norm()), float(g.norm())
    r = 1.0
    if adapt and wn > 0 and gn > 0:
        r = eta * wn / (gn + wd * wn + eps)
        if trust_clip:
            r = min(r / lr, 1.0)
    gi = (g + wd * p) * r
    G = (g.abs() + wd * p.abs()) * r
    if mu != 0:
        nbuf = mu * buf + gi
        B = mu * buf.abs() + G
        d = gi + mu * nbuf if nesterov else nbuf
        D = G + mu * B if nesterov else B
    else:
        nbuf, B, d, D = buf, buf.abs(), gi, G
    return p - lr * d, nbuf, r, D, B


SHAPES = [(7, 5), (33,), (3, 4, 2, 2), (1,), (64, 9)]


@pytest.mark.parametrize("trust_clip", [False, True])
@pytest.mark.parametrize("mu,nesterov", [(0.0, False), (0.9, False),
                                         (0.9, True)])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_cpu_path_equals_float64_formula(wd, mu, nesterov, trust_clip):
    """The CPU path takes both norms in float64 and rounds the ratio to fp32
    once (1 rounding).  The fp32 chain after it is at most: g + wd*p (2),
    * r (1), mu*buf + gi (2), gi + mu*buf (2), p - lr*d (2) = 9 roundings,
    10 with the ratio's.  Each is at most U = 2**-24 relative to a value
    bounded by the absolute-value chain (|p| + lr*D for p, B for buf), so
    |p - p_ref| <= 10*U*(|p| + lr*D) and |buf - buf_ref| <= 6*U*B."""
    from ddp_tricks_amd.ops.optim import FusedLARS
    lr, eta, eps = 0.1, 0.02, 1e-8
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    gs = [torch.randn(s, generator=g) * 3.0 for s in SHAPES]
    b0 = [torch.randn(s, generator=g) * 0.1 for s in SHAPES]
    p0 = [p.detach().clone() for p in ps]
    opt = FusedLARS(ps, lr=lr, momentum=mu, weight_decay=wd,
                    nesterov=nesterov, trust_coefficient=eta, eps=eps,
                    trust_clip=trust_clip)
    for p, gr, b in zip(ps, gs, b0):
        p.grad = gr.clone()
        if mu != 0:
            opt.state[p]["momentum_buffer"] = b.clone()
    opt.step()
    assert opt.trust_ratios.dtype == torch.float32
    assert opt.trust_ratios.shape == (len(SHAPES),)
    for i, (p, gr, b) in enumerate(zip(ps, gs, b0)):
        rp, rb, r, D, B = _ref_step(p0[i], gr, b, lr, mu, wd, nesterov, eta,
                                    eps, trust_clip)
        assert abs(float(opt.trust_ratios[i]) - r) <= U * r, i
        bound = 10 * U * (p0[i].double().abs() + lr * D)
        assert bool(((p.detach().double() - rp).abs() <= bound).all()), i
        if mu != 0:
            got = opt.state[p]["momentum_buffer"].double()
            assert bool(((got - rb).abs() <= 6 * U * B).all()), i
        else:
            assert "momentum_buffer" not in opt.state[p]
        assert not torch.equal(p.detach(), p0[i])            # it stepped


def test_cpu_degenerate_and_mixed_groups():
    """Zero gradient / zero parameter tensors get ratio 1; a non-adapted
    group takes exactly the FusedSGD step; trust_ratios is allocated once
    and follows the parameter order across groups."""
    from ddp_tricks_amd.ops.optim import FusedLARS, FusedSGD
    g = torch.Generator().manual_seed(6)

    def make():
        gen = torch.Generator().manual_seed(7)
        a = [torch.nn.Parameter(torch.randn(6, 3, generator=gen)),
             torch.nn.Parameter(torch.zeros(5, 2)),
             torch.nn.Parameter(torch.randn(4, 4, generator=gen))]
        b = [torch.nn.Parameter(torch.randn(9, generator=gen)),
             torch.nn.Parameter(torch.randn(3, generator=gen))]
        return a, b
    a, b = make()
    a2, b2 = make()
    grads = [torch.randn(p.shape, generator=g) for p in a + b]
    grads[2].zero_()
    lars = FusedLARS([dict(params=a, weight_decay=5e-4),
                      dict(params=b, adapt=False, weight_decay=0.0)],
                     lr=0.1, momentum=0.9, nesterov=True,
                     trust_coefficient=0.01)
    sgd = FusedSGD(b2, lr=0.1, momentum=0.9, nesterov=True)
    for p, gr in zip(a + b, grads):
        p.grad = gr.clone()
    for p, gr in zip(b2, grads[3:]):
        p.grad = gr.clone()
    for step in range(2):
        lars.step()
        sgd.step()
        ratios = lars.trust_ratios
        # a[1] was all zero before the first step only; a[2]'s gradient is
        # zero throughout
        assert ratios.tolist()[2:] == [1.0, 1.0, 1.0]
        assert (float(ratios[1]) == 1.0) == (step == 0)
        assert 0.0 < float(ratios[0]) < 1.0
    assert lars.trust_ratios is ratios                       # reused
    for p, q in zip(b, b2):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(lars.state[p]["momentum_buffer"],
                           sgd.state[q]["momentum_buffer"])
    assert all(bool(torch.isfinite(p).all()) for p in a + b)
    # a parameter without a gradient is left alone; its neighbours step
    before = [p.detach().clone() for p in a]
    a[1].grad = None
    a[2].grad = torch.ones(4, 4)
    lars.step()
    assert torch.equal(a[1].detach(), before[1])
    assert not torch.equal(a[0].detach(), before[0])
    assert not torch.equal(a[2].detach(), before[2])
    assert 0.0 < float(lars.trust_ratios[2]) < 1.0
    # zero_grad keeps the storage
    ptr = a[0].grad.data_ptr()
    lars.zero_grad()
    assert a[0].grad.data_ptr() == ptr and not bool(a[0].grad.any())


def test_constructor_validation():
    from ddp_tricks_amd import ops
    from ddp_tricks_amd.ops.optim import FusedLARS
    assert ops.FusedLARS is FusedLARS
    p = [torch.nn.Parameter(torch.ones(2, 2))]
    with pytest.raises(ValueError):
        FusedLARS(p, lr=-1.0)
    with pytest.raises(ValueError):
        FusedLARS(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedLARS(p, lr=0.1, trust_coefficient=0.0)
    opt = FusedLARS(p, lr=0.1)
    assert opt.param_groups[0]["adapt"] is True
    assert opt.param_groups[0]["trust_coefficient"] == 0.001
    assert opt.param_groups[0]["eps"] == 1e-8
    assert opt.param_groups[0]["trust_clip"] is False


@pytest.mark.parametrize("name", ["toy_net", "resnet18"])
def test_lars_param_groups_split(name):
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops import lars_param_groups
    model = build_model(name)
    groups = lars_param_groups(model, 5e-4)
    assert len(groups) == 2
    adapted, plain = groups
    assert adapted["adapt"] is True and adapted["weight_decay"] == 5e-4
    assert plain["adapt"] is False and plain["weight_decay"] == 0.0
    assert adapted["params"] and plain["params"]
    assert all(p.ndim > 1 for p in adapted["params"])
    assert all(p.ndim <= 1 for p in plain["params"])
    got = [id(p) for g in groups for p in g["params"]]
    want = [id(p) for p in model.parameters()]
    assert len(got) == len(set(got)) == len(want)
    assert set(got) == set(want)
    # every BatchNorm parameter and every bias is in the plain group
    plain_ids = {id(p) for p in plain["params"]}
    for n, p in model.named_parameters():
        if n.endswith(".bias") or "bn" in n.split(".")[-2]:
            assert id(p) in plain_ids, n


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


def _worker_stack(rank, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from ddp_tricks_amd.ops.optim import FusedLARS, lars_param_groups
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    from ddp_tricks_amd.utils.lookahead import Lookahead
    amp._state.__init__()
    torch.manual_seed(7)
    model = _Net()
    opt = FusedLARS(lars_param_groups(model, 5e-4), lr=0.1, momentum=0.9,
                    nesterov=True, trust_coefficient=0.02)
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
        sigs.append(([p.detach().numpy().tobytes()
                      for p in model.parameters()],
                     opt.trust_ratios.numpy().tobytes(),
                     opt.trust_ratios.tolist()))
    n_adapted = len(opt.param_groups[0]["params"])
    amp._state.__init__()
    results.put((rank, (sigs, n_adapted)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_world2_full_stack_in_bitwise_lockstep():
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=_worker_stack, args=(r, 29636, results))
             for r in range(WORLD)]
    [p.start() for p in procs]
    got = dict(results.get(timeout=110) for _ in range(WORLD))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    (s0, n_adapted), (s1, _) = got[0], got[1]
    for step in range(4):
        assert s0[step][0] == s1[step][0], f"params differ at step {step}"
        assert s0[step][1] == s1[step][1], f"ratios differ at step {step}"
        ratios = s0[step][2]
        assert all(0.0 < r < float("inf") for r in ratios[:n_adapted])
        assert ratios[n_adapted:] == [1.0] * (len(ratios) - n_adapted)
    assert n_adapted == 3 and len(s0[0][2]) == 10
    assert s0[0][0] != s0[3][0]                              # it trained
    assert s0[0][1] != s0[3][1]


# ------------------------------------------------------------- trainer flags ---

def _load_run():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_lars", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_flags(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    a = run.parse_args()
    assert (a.optimizer, a.weight_decay, a.lars_eta) == ("sgd", 0.0, 0.001)
    monkeypatch.setattr(sys, "argv", ["run.py", "--optimizer", "lars",
                                      "--weight_decay", "5e-4",
                                      "--lars_eta", "0.02", "--resume"])
    a = run.parse_args()
    assert (a.optimizer, a.weight_decay, a.lars_eta) == ("lars", 5e-4, 0.02)
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
        os.environ.setdefault("MASTER_PORT", "29637")
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


def test_default_flags_build_the_same_fused_sgd(tmp_path, monkeypatch,
                                                dist_env):
    from ddp_tricks_amd.ops.optim import FusedLARS, FusedSGD
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    opt, kw = _built_optimizer(tmp_path, monkeypatch)
    assert type(opt) is FusedSGD and not isinstance(opt, FusedLARS)
    assert kw == dict(k=10, alpha=0.5)
    assert len(opt.param_groups) == 1
    grp = opt.param_groups[0]
    assert grp["weight_decay"] == 0
    assert (grp["lr"], grp["momentum"], grp["nesterov"]) == (0.05, 0.9, True)
    assert "adapt" not in grp and "trust_coefficient" not in grp


def test_lars_flags_build_fused_lars(tmp_path, monkeypatch, dist_env):
    from ddp_tricks_amd.ops.optim import FusedLARS
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    opt, kw = _built_optimizer(tmp_path, monkeypatch, optimizer="lars",
                               weight_decay=5e-4, lars_eta=0.02)
    assert type(opt) is FusedLARS and kw == dict(k=10, alpha=0.5)
    adapted, plain = opt.param_groups
    assert adapted["adapt"] is True and adapted["weight_decay"] == 5e-4
    assert plain["adapt"] is False and plain["weight_decay"] == 0.0
    for grp in opt.param_groups:
        assert grp["trust_coefficient"] == 0.02
        assert (grp["momentum"], grp["nesterov"]) == (0.9, True)
    with pytest.raises(ValueError, match="unknown optimizer"):
        _built_optimizer(tmp_path, monkeypatch, optimizer="adam")


@pytest.mark.timeout(300)
def test_lars_resume_bitwise_equals_straight_run(tmp_path, monkeypatch,
                                                 dist_env):
    """`run.py --optimizer lars --weight_decay 5e-4 --resume`: 2 epochs +
    resume for 2 more equals 4 straight epochs, bit for bit (the optimizer
    state is the momentum buffers alone)."""
    from ddp_tricks_amd.utils.train import train
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "256")
    lars = dict(resume=True, optimizer="lars", weight_decay=5e-4)

    amp._state.__init__()
    train(_args(tmp_path, "STRAIGHT", 4, **lars))
    ck = torch.load(os.path.join(tmp_path, "STRAIGHT.resume.pt"),
                    weights_only=False)
    straight = ck["model"]
    groups = ck["optimizer"]["param_groups"]
    assert [g["adapt"] for g in groups] == [True, False]
    assert [g["weight_decay"] for g in groups] == [5e-4, 0.0]
    for st in ck["optimizer"]["fast_state"].values():
        assert set(st) == {"momentum_buffer"}

    amp._state.__init__()
    train(_args(tmp_path, "SPLIT", 2, **lars))
    amp._state.__init__()
    train(_args(tmp_path, "SPLIT", 4, **lars))
    amp._state.__init__()
    split = torch.load(os.path.join(tmp_path, "SPLIT.resume.pt"),
                       weights_only=False)["model"]
    for k in straight:
        assert torch.equal(straight[k], split[k]), k
        assert bool(torch.isfinite(straight[k]).all()), k

    # the lars run is a different trajectory from the default sgd one
    amp._state.__init__()
    train(_args(tmp_path, "SGD", 4, resume=True))
    amp._state.__init__()
    sgd = torch.load(os.path.join(tmp_path, "SGD.resume.pt"),
                     weights_only=False)["model"]
    assert any(not torch.equal(straight[k], sgd[k]) for k in straight)
