"""SyncBatchNorm on the CPU tier: the plain-torch path over gloo against a
float64 full-batch reference, the in-place conversion, the converted model
under this project's DDP + amp + FusedSGD + Lookahead stack, and the CLI
switch."""
import os
import re
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from ddp_tricks_amd import amp

WORLD = 2
ATOL = 1e-5     # tests/test_ddp_gloo.py's gradient-equivalence tolerance
SPLIT = (5, 3)  # unequal shards of the 8-sample batch


def _init(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)


def _case(shape):
    g = torch.Generator().manual_seed(1234 + len(shape))
    C = shape[1]
    x = torch.randn(shape, generator=g) * 2.0 + 0.5
    t = torch.randn(shape, generator=g)
    r = torch.randn(shape, generator=g)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    rm0 = torch.randn(C, generator=g)
    rv0 = torch.rand(C, generator=g) + 0.5
    return x, t, r, w, b, rm0, rv0


CASES = [((8, 6, 5, 3), False), ((8, 6, 5, 3), True), ((8, 10), False),
         ((8, 10), True)]


def _worker_equiv(rank, port, results):
    _init(rank, port)
    from ddp_tricks_amd.ops.modules import SyncBatchNorm
    lo = sum(SPLIT[:rank])
    hi = lo + SPLIT[rank]
    out = []
    for shape, fused in CASES:
        x, t, r, w, b, rm0, rv0 = _case(shape)
        bn = SyncBatchNorm(shape[1], fuse_relu=fused)
        with torch.no_grad():
            bn.weight.copy_(w)
            bn.bias.copy_(b)
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
        bn.train()
        xs = x[lo:hi].clone().requires_grad_(True)
        if len(shape) == 4:
            y = bn(xs, residual=r[lo:hi] if fused else None)
        else:
            y = bn(xs)
        (y * t[lo:hi]).sum().backward()
        gw, gb = bn.weight.grad.clone(), bn.bias.grad.clone()
        dist.all_reduce(gw)
        dist.all_reduce(gb)
        # eval mode: the plain path on the synchronised running statistics
        bn.eval()
        with torch.no_grad():
            ye = bn(x[lo:hi])
        out.append(dict(y=y.detach().numpy(), dx=xs.grad.numpy(),
                        gw=gw.numpy(), gb=gb.numpy(), ye=ye.numpy(),
                        rm=bn.running_mean.numpy().copy(),
                        rv=bn.running_var.numpy().copy(),
                        nbt=int(bn.num_batches_tracked)))
    results.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(target, port, n=WORLD, timeout=110):
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, port, results))
             for r in range(n)]
    [p.start() for p in procs]
    got = dict(results.get(timeout=timeout) for _ in range(n))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    return got


@pytest.mark.timeout(180)
def test_world2_matches_float64_full_batch():
    got = _spawn(_worker_equiv, 29631)
    for i, (shape, fused) in enumerate(CASES):
        x, t, r, w, b, rm0, rv0 = _case(shape)
        use_r = fused and len(shape) == 4
        xd = x.double().requires_grad_(True)
        wd = w.double().requires_grad_(True)
        bd = b.double().requires_grad_(True)
        rm, rv = rm0.double(), rv0.double()
        y = F.batch_norm(xd, rm, rv, wd, bd, True, 0.1, 1e-5)
        if use_r:
            y = y + r.double()
        if fused:
            y = F.relu(y)
        (y * t.double()).sum().backward()
        ye = F.batch_norm(x.double(), rm, rv, wd.detach(), bd.detach(),
                          False, 0.1, 1e-5)
        if fused:
            ye = F.relu(ye)
        for rank in range(WORLD):
            lo = sum(SPLIT[:rank])
            hi = lo + SPLIT[rank]
            o = got[rank][i]
            what = (shape, fused, rank)

            def close(a, ref):
                return torch.allclose(torch.from_numpy(a).double(), ref,
                                      rtol=0, atol=ATOL)
            assert close(o["y"], y.detach()[lo:hi]), what
            assert close(o["dx"], xd.grad[lo:hi]), what
            assert close(o["gw"], wd.grad), what
            assert close(o["gb"], bd.grad), what
            assert close(o["rm"], rm), what
            assert close(o["rv"], rv), what
            assert close(o["ye"], ye[lo:hi]), what
            assert o["nbt"] == 1
        # both ranks hold the same buffers, bit for bit
        for k in ("rm", "rv"):
            assert got[0][i][k].tobytes() == got[1][i][k].tobytes(), (shape, k)
        # the statistics really are global: the rank-local ones differ
        local = x[:SPLIT[0]].double().transpose(0, 1).reshape(shape[1], -1)
        assert not torch.allclose(0.9 * rm0.double() + 0.1 * local.mean(1),
                                  rm, atol=1e-3)


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


def test_convert_keeps_parameters_flags_and_keys():
    from ddp_tricks_amd import parallel
    from ddp_tricks_amd.ops.modules import BatchNorm2d, SyncBatchNorm
    assert parallel.convert_syncbn_model is parallel.convert_sync_batchnorm
    torch.manual_seed(3)
    net = _Net()
    keys = list(net.state_dict().keys())
    before = {k: v for k, v in list(net.named_parameters())
              + list(net.named_buffers())}
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(6, 1, 4, 4)
    net.train()
    y0 = net(x)
    net.load_state_dict(sd)         # undo the running-stat update
    out = parallel.convert_sync_batchnorm(net)
    assert out is net
    assert isinstance(net.bn, SyncBatchNorm) and net.bn.fuse_relu is True
    assert isinstance(net.bn1, SyncBatchNorm) and net.bn1.fuse_relu is False
    assert list(net.state_dict().keys()) == keys
    after = {k: v for k, v in list(net.named_parameters())
             + list(net.named_buffers())}
    assert before.keys() == after.keys()
    for k in before:
        assert after[k] is before[k], k
    # no process group (or one of a single rank, if an earlier test of the
    # session left it): the plain path, bit for bit
    assert not dist.is_initialized() or dist.get_world_size() == 1
    assert torch.equal(net(x), y0)
    # a checkpoint of the plain model loads into the converted one
    net.load_state_dict(sd)
    # a bare BatchNorm root is converted too
    root = parallel.convert_sync_batchnorm(BatchNorm2d(8, fuse_relu=True))
    assert isinstance(root, SyncBatchNorm) and root.fuse_relu
    # eval mode and input rank checks
    with pytest.raises(ValueError):
        root(torch.zeros(2, 8, 3))
    root.eval()
    assert root(torch.zeros(2, 8, 3, 3)).shape == (2, 8, 3, 3)


def _worker_stack(rank, port, results):
    """tests/test_ddp_gloo.py's production wiring on a converted model."""
    _init(rank, port)
    from ddp_tricks_amd.ops.modules import SyncBatchNorm
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.parallel import convert_sync_batchnorm
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    from ddp_tricks_amd.utils.lookahead import Lookahead
    amp._state.__init__()
    torch.manual_seed(7)
    model = convert_sync_batchnorm(_Net())
    assert isinstance(model.bn, SyncBatchNorm)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    la = Lookahead(opt, k=2, alpha=0.5)
    model, apex_opt = amp.initialize(model, la, "O1")
    ddp = DDP(model)
    assert model.bn._native_comm is None      # CPU: process-group transport
    torch.manual_seed(500 + rank)             # DIFFERENT data per rank
    sigs = []
    for step in range(3):
        apex_opt.zero_grad()
        x = torch.randn(4 + rank, 1, 4, 4)    # unequal local batches
        t = torch.randn(4 + rank, 3)
        ddp.train()
        loss = ((ddp(x) - t) ** 2).mean()
        with amp.scale_loss(loss, apex_opt) as sl:
            sl.backward()
        # buffers BEFORE the next forward's rank-0 broadcast: the sync
        # update itself must leave them rank-identical
        bsig = [b.detach().numpy().tobytes() for b in model.buffers()]
        gsig = [p.grad.numpy().tobytes() for p in model.parameters()]
        apex_opt.step()
        psig = [p.detach().numpy().tobytes() for p in model.parameters()]
        sigs.append((bsig, gsig, psig))
    amp._state.__init__()
    results.put((rank, sigs))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_converted_model_trains_in_bitwise_lockstep_under_ddp():
    got = _spawn(_worker_stack, 29632)
    for step in range(3):
        for kind, a, b in zip(("buffers", "grads", "params"),
                              got[0][step], got[1][step]):
            assert a == b, f"{kind} differ across ranks at step {step}"
    # the parameters moved
    assert got[0][0][2] != got[0][2][2]


def _load_run():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_syncbn", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_sync_bn_flag(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    assert run.parse_args().sync_bn is False
    monkeypatch.setattr(sys, "argv", ["run.py", "--sync_bn"])
    assert run.parse_args().sync_bn is True


def _train_args(tmp_path, name, **over):
    a = types.SimpleNamespace(
        exp_name=name, learning_rate=0.1, batch_size=64, epochs=2,
        warmup_epochs=1, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _epoch_lines(out):
    lines = [l for l in out.splitlines() if l.startswith("epoch:")]
    return [re.sub(r"time: [0-9.]+s, ", "", l) for l in lines]


@pytest.mark.timeout(300)
def test_trainer_sync_bn_one_process_prints_the_same_epochs(
        tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29633")
        dist.init_process_group("gloo", rank=0, world_size=1)
    import importlib
    # (the package re-exports the train() function under the module's name)
    train_mod = importlib.import_module("ddp_tricks_amd.utils.train")
    seen = []
    real = train_mod.DDP

    def spy(model, *a, **k):
        seen.append(sum(getattr(m, "is_sync_bn", False)
                        for m in model.modules()))
        return real(model, *a, **k)
    monkeypatch.setattr(train_mod, "DDP", spy)
    # a CPU run wherever the suite runs (on a GPU the converted model's
    # BN+pool junctions run unfused, which reorders fp32 sums)
    monkeypatch.setattr(train_mod, "_resolve_device",
                        lambda local_rank: torch.device("cpu"))
    try:
        amp._state.__init__()
        train_mod.train(_train_args(tmp_path, "SYNCBN_on", sync_bn=True))
        out_on = capsys.readouterr().out
        amp._state.__init__()
        train_mod.train(_train_args(tmp_path, "SYNCBN_off"))
        out_off = capsys.readouterr().out
    finally:
        amp._state.__init__()
        dist.destroy_process_group()
    assert seen == [5, 0]           # Toy_Net's five BatchNorms, converted
    on, off = _epoch_lines(out_on), _epoch_lines(out_off)
    assert len(on) == 2 and on == off
