"""Global gradient-norm clipping, CPU tier: the clip_grad_norm_ formula, the
amp sync / O0 branches, update-size bounds through FusedSGD, off-means-off,
world-2 gloo lockstep and the trainer's --clip_grad_norm telemetry."""
import math
import os
import re
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddp_tricks_amd import amp, same_seeds
from ddp_tricks_amd.ops import clip_grad_norm_
from ddp_tricks_amd.ops.optim import FusedSGD
from ddp_tricks_amd.utils.lookahead import Lookahead

WORLD = 2


@pytest.fixture(autouse=True)
def _reset_amp():
    amp._state.__init__()
    yield
    amp._state.__init__()


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(8, 16)
        self.bn = torch.nn.BatchNorm1d(16)
        self.fc2 = torch.nn.Linear(16, 4)

    def forward(self, x):
        return self.fc2(torch.relu(self.bn(self.fc1(x))))


def _tensor_list(seed=0):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(40, generator=g)
    return [torch.zeros(0),                     # 0-element tensor
            flat.narrow(0, 3, 17),              # offset view of a flat
            torch.randn(1, generator=g),        # 1-element tensor
            torch.randn(5, 7, generator=g)], flat


def _norm64(tensors):
    return math.sqrt(sum(float(t.double().pow(2).sum()) for t in tensors))


def _coef32(max_norm, norm):
    """torch's clip_grad_norm_ coefficient in fp32 arithmetic."""
    n32 = torch.tensor(norm, dtype=torch.float32)
    return float((max_norm / (n32 + 1e-6)).clamp(max=1.0))


# ------------------------------------------------ clip_grad_norm_ formula ---

def test_clip_formula_scales_above_threshold():
    ts, flat = _tensor_list()
    before = [t.clone() for t in ts]
    flat_before = flat.clone()
    norm = _norm64(ts)
    max_norm = 0.25 * norm
    got = clip_grad_norm_(ts, max_norm)
    assert got.dim() == 0 and got.dtype == torch.float32
    assert float(got) == pytest.approx(norm, rel=1e-6)
    coef = _coef32(max_norm, norm)
    assert coef < 1
    for t, b in zip(ts, before):
        assert torch.allclose(t, b * coef, rtol=1e-6, atol=0)
    assert _norm64(ts) <= max_norm * (1 + 1e-6)
    # the view was scaled inside its flat; the rest of the flat is untouched
    assert torch.equal(flat[:3], flat_before[:3])
    assert torch.equal(flat[20:], flat_before[20:])
    assert torch.equal(flat[3:20], ts[1])


def test_clip_untouched_at_or_below_threshold():
    # below: any max_norm above the norm
    ts, _ = _tensor_list(1)
    before = [t.clone() for t in ts]
    norm = _norm64(ts)
    got = clip_grad_norm_(ts, 2.0 * norm)
    assert float(got) == pytest.approx(norm, rel=1e-6)
    for t, b in zip(ts, before):
        assert torch.equal(t, b)
    # at: 16384 ones have norm exactly 128 == max_norm (128 + 1e-6 rounds
    # to 128 in fp32, so the formula's coefficient is exactly 1)
    ones = [torch.ones(16000), torch.ones(384)]
    got = clip_grad_norm_(ones, 128.0)
    assert float(got) == 128.0
    assert all(bool((t == 1).all()) for t in ones)


def test_clip_accepts_parameters_and_measures_with_zero():
    p = torch.nn.Parameter(torch.zeros(6))
    q = torch.nn.Parameter(torch.zeros(3))      # no grad: ignored
    p.grad = torch.full((6,), 2.0)
    n = clip_grad_norm_([p, q], 1.0)
    assert float(n) == pytest.approx(math.sqrt(24.0), rel=1e-6)
    assert _norm64([p.grad]) <= 1.0 * (1 + 1e-6)
    g = torch.full((4,), 3.0)
    n = clip_grad_norm_(g, 0.0)                 # single tensor, measure only
    assert float(n) == 6.0 and bool((g == 3.0).all())
    assert float(clip_grad_norm_([], 1.0)) == 0.0


# ------------------------------------------------------------ amp paths ---

def _amp_setup(opt_level="O1", max_grad_norm=None, lr=0.1, momentum=0.9,
               nesterov=True, seed=3):
    same_seeds(seed)
    model = TinyNet()
    opt = FusedSGD(model.parameters(), lr=lr, momentum=momentum,
                   nesterov=nesterov)
    model, opt = amp.initialize(model, opt, opt_level=opt_level,
                                max_grad_norm=max_grad_norm)
    return model, opt


def _backward(model, opt, seed=5, big=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, 8, generator=g)
    t = torch.randn(8, 4, generator=g)
    opt.zero_grad()
    model.train()
    loss = big * ((model(x) - t) ** 2).mean()
    with amp.scale_loss(loss, opt) as sl:
        sl.backward()


def _grads(opt):
    return [p.grad for g in opt.param_groups for p in g["params"]
            if p.grad is not None]


def test_amp_sync_path_clips():
    m = 1e-2
    model, opt = _amp_setup(max_grad_norm=None)
    _backward(model, opt)
    unclipped = _norm64(_grads(opt))
    assert unclipped > m
    assert amp.last_grad_norm() is None
    model, opt = _amp_setup(max_grad_norm=m)
    _backward(model, opt)
    assert _norm64(_grads(opt)) <= m * (1 + 1e-6)
    # the reported norm is the pre-clip one
    assert float(amp.last_grad_norm()) == pytest.approx(unclipped, rel=1e-5)
    assert amp.pending_grad_scale() is None      # CPU: clipped in place
    st = amp.pop_grad_norm_stats()
    assert st["steps"] == 1 and st["clipped_frac"] == 1.0
    assert st["mean"] == pytest.approx(unclipped, rel=1e-5)
    assert st["max"] == pytest.approx(unclipped, rel=1e-5)
    assert amp.pop_grad_norm_stats()["steps"] == 0   # pop resets


def test_amp_sync_path_overflow():
    model, opt = _amp_setup(max_grad_norm=1e-2)
    _backward(model, opt)
    opt.step()
    assert amp.pop_grad_norm_stats()["steps"] == 1
    before = [p.detach().clone() for p in model.parameters()]
    scale0 = amp.state().scaler.scale
    # plant an inf through a backward hook
    h = model.fc2.weight.register_hook(
        lambda g: torch.where(torch.arange(g.numel()).reshape(g.shape) == 5,
                              torch.full_like(g, float("inf")), g))
    _backward(model, opt)
    h.remove()
    opt.step()                                   # skipped
    assert amp.state().scaler.scale == scale0 / 2
    assert not math.isfinite(float(amp.last_grad_norm()))
    for p, b in zip(model.parameters(), before):
        assert torch.equal(p.detach(), b)
    st = amp.pop_grad_norm_stats()
    assert st["steps"] == 0 and st["clipped_frac"] == 0.0


def test_amp_o0_branch_clips():
    m = 1e-2
    model, opt = _amp_setup(opt_level="O0", max_grad_norm=m)
    _backward(model, opt)
    assert 0 < _norm64(_grads(opt)) <= m * (1 + 1e-6)
    assert float(amp.last_grad_norm()) > m
    assert amp.pop_grad_norm_stats()["steps"] == 1


# ---------------------------------------------------------- update size ---

@pytest.mark.parametrize("scale,clips", [(1e3, True), (1e-6, False)])
def test_update_size(scale, clips):
    m = 1e-2
    model, opt = _amp_setup(max_grad_norm=m, lr=1.0, momentum=0.0,
                            nesterov=False)
    before = [p.detach().clone() for p in model.parameters()]
    _backward(model, opt, big=scale)
    g = [x.clone() for x in _grads(opt)]
    opt.step()
    delta = [p.detach() - b for p, b in zip(model.parameters(), before)]
    norm = float(amp.last_grad_norm())
    if clips:
        assert norm > 100 * m
        assert _norm64(delta) <= m * (1 + 1e-5)
    else:
        assert norm < m / 100
        for p, b, gi in zip(model.parameters(), before, g):
            assert torch.equal(p.detach(), b - gi)


# ------------------------------------------------------- off means off ---

def _three_steps(max_grad_norm):
    amp._state.__init__()
    same_seeds(9)
    model = TinyNet()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    la = Lookahead(opt, k=2, alpha=0.5)
    model, la = amp.initialize(model, la, "O1", max_grad_norm=max_grad_norm)
    g = torch.Generator().manual_seed(2)
    pend = []
    for _ in range(3):
        la.zero_grad()
        x = torch.randn(8, 8, generator=g)
        t = torch.randn(8, 4, generator=g)
        loss = ((model(x) - t) ** 2).mean()
        with amp.scale_loss(loss, la) as sl:
            sl.backward()
        pend.append(amp.pending_grad_scale())
        la.step()
    return [p.detach().clone() for p in model.parameters()], pend


def test_off_means_off():
    p_none, pend_none = _three_steps(None)
    p_zero, pend_zero = _three_steps(0)
    assert all(x is None for x in pend_none + pend_zero)
    for a, b in zip(p_none, p_zero):
        assert torch.equal(a, b)
    assert amp.last_grad_norm() is None


# ------------------------------------------------------- world-2 gloo ---

CLIP_M = 1e-2


def _worker_clip(rank, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    amp._state.__init__()
    torch.manual_seed(7)
    model = TinyNet()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    la = Lookahead(opt, k=2, alpha=0.5)
    model, apex_opt = amp.initialize(model, la, "O1", max_grad_norm=CLIP_M)
    ddp = DDP(model, bucket_cap_mb=0.0001)
    torch.manual_seed(123)               # same generator state on both ranks
    norms = []
    for _ in range(3):
        apex_opt.zero_grad()
        x = torch.randn(WORLD * 4, 8)
        t = torch.randn(WORLD * 4, 4)
        ddp.train()
        sl_ = slice(rank * 4, (rank + 1) * 4)    # DIFFERENT data per rank
        loss = ((ddp(x[sl_]) - t[sl_]) ** 2).mean()
        with amp.scale_loss(loss, apex_opt) as sl:
            sl.backward()
        norms.append(amp.last_grad_norm().clone().numpy())
        apex_opt.step()
    stats = amp.pop_grad_norm_stats()
    amp._state.__init__()
    results.put((rank, [n.tobytes() for n in norms],
                 {k: p.detach().numpy().copy()
                  for k, p in model.named_parameters()}, stats))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_world2_clip_lockstep_and_fullbatch_equivalence():
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=_worker_clip, args=(r, 29631, results))
             for r in range(WORLD)]
    [p.start() for p in procs]
    got = {}
    for _ in range(WORLD):
        r, norms, params, stats = results.get(timeout=110)
        got[r] = (norms, params, stats)
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    # bitwise lockstep: norms and parameters
    assert got[0][0] == got[1][0]
    for k in got[0][1]:
        assert got[0][1][k].tobytes() == got[1][1][k].tobytes(), k
    assert got[0][2]["steps"] == 3 and got[0][2]["clipped_frac"] == 1.0

    # single-process oracle: clip the averaged full-batch gradient.  Each
    # rank's BN sees only its shard, so the oracle runs one replica per
    # shard (shared weights), averages the two gradients, then clips.
    amp._state.__init__()
    torch.manual_seed(7)
    model = TinyNet()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    la = Lookahead(opt, k=2, alpha=0.5)
    torch.manual_seed(123)
    import copy
    for _ in range(3):
        x = torch.randn(WORLD * 4, 8)
        t = torch.randn(WORLD * 4, 4)
        model.train()
        grads = None
        for r in range(WORLD):
            rep = copy.deepcopy(model) if r else model
            rep.zero_grad()
            sl_ = slice(r * 4, (r + 1) * 4)
            ((rep(x[sl_]) - t[sl_]) ** 2).mean().backward()
            gr = [p.grad.clone() for p in rep.parameters()]
            grads = gr if grads is None else [a + b for a, b in zip(grads, gr)]
        for p, g in zip(model.parameters(), grads):
            p.grad = g / WORLD
        n = clip_grad_norm_([p.grad for p in model.parameters()], CLIP_M)
        assert float(n) > CLIP_M                 # every step clips
        la.step()
    for k, p in model.named_parameters():
        assert torch.allclose(torch.from_numpy(got[0][1][k]), p.detach(),
                              atol=1e-5), k


# ------------------------------------------------------------- trainer ---

def _train_args(tmp_path, name, **over):
    a = types.SimpleNamespace(
        exp_name=name, learning_rate=0.1, batch_size=64, epochs=2,
        warmup_epochs=1, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _tfevents_bytes(logdir):
    blob = b""
    for root, _, files in os.walk(logdir):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                blob += fh.read()
    return blob


@pytest.mark.timeout(300)
def test_trainer_clip_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29657")
        dist.init_process_group("gloo", rank=0, world_size=1)
    from ddp_tricks_amd.utils.train import train
    try:
        train(_train_args(tmp_path, "CLIP_on", clip_grad_norm=1e-3))
        out_on = capsys.readouterr().out
        amp._state.__init__()
        train(_train_args(tmp_path, "CLIP_off"))
        out_off = capsys.readouterr().out
    finally:
        dist.destroy_process_group()
    lines_on = [l for l in out_on.splitlines() if l.startswith("epoch:")]
    assert len(lines_on) == 2
    for l in lines_on:
        assert re.search(r", grad_norm: \d+\.\d{4}, clipped: \d+\.\d%$", l), l
    # epoch 1 trains at LR > 0 with a 1e-3 bound: every step clips
    assert lines_on[1].endswith("clipped: 100.0%")
    ev_on = _tfevents_bytes(os.path.join(tmp_path, "logs", "CLIP_on"))
    assert b"GradNorm" in ev_on and b"GradClipFrac" in ev_on
    assert "grad_norm:" not in out_off and "clipped:" not in out_off
    ev_off = _tfevents_bytes(os.path.join(tmp_path, "logs", "CLIP_off"))
    assert b"GradNorm" not in ev_off and b"GradClipFrac" not in ev_off
    assert b"LR" in ev_off


def test_run_py_flag_default(monkeypatch):
    import importlib.util
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    monkeypatch.setattr(sys, "argv", ["run.py"])
    assert run.parse_args().clip_grad_norm == 0.0
    monkeypatch.setattr(sys, "argv", ["run.py", "--clip_grad_norm", "0.5"])
    assert run.parse_args().clip_grad_norm == 0.5
