"""Counter-hash dropout without a GPU: the threshold, the numpy mirror of the
kernels' mask, the host-side call-seed stream, the CPU path of
``linear_relu_dropout`` / ``Dropout`` and the ``run.py --dropout`` plumbing.

The statistical checks are caps, not measurements.  A mask of n elements at
drop probability q = thr/65536 has a Binomial(n, q) dropped count; over the
60 (seed, p) cases below |z| <= 4.5 fails a sound generator with
probability < 1e-3 (observed: at most 1.8).  Two independent p = 0.5 masks
agree on a Binomial(2^20, 0.5) count of elements: sigma = 0.0005 of the
fraction, the +-0.005 window is 10 sigma (observed 0.4998 and 0.5001).
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

from ddp_tricks_amd import amp, ops
from ddp_tricks_amd.ops import functional as Fo
from ddp_tricks_amd.ops.functional import (DropoutRNG, dropout_mask,
                                           dropout_scale, dropout_threshold)


@pytest.fixture(autouse=True)
def _fresh_rng():
    """Every test starts from, and leaves, the same singleton state."""
    saved = ops.dropout_rng.state_dict()
    ops.dropout_rng.seed(1234, rank=0)
    yield
    ops.dropout_rng.load_state_dict(saved)


# -------------------------------------------------------------- threshold ---

def test_threshold_edges_and_rejections():
    assert dropout_threshold(0.0) == 0
    assert dropout_threshold(0.5) == 32768
    assert dropout_threshold(0.75) == 49152
    assert dropout_threshold(0.1) == 6554          # floor(6553.6 + 0.5)
    assert dropout_threshold(1.0 / 131072) == 1    # exactly .5 rounds up
    assert dropout_threshold(0.4999 / 65536) == 0
    assert dropout_threshold(65535.0 / 65536) == 65535
    assert dropout_threshold(65535.4 / 65536) == 65535
    for bad in (-0.1, -1e-9, 1.0, 65535.5 / 65536, 1.5, float("nan"),
                float("inf")):
        with pytest.raises(ValueError):
            dropout_threshold(bad)
    assert dropout_scale(0) == 1.0
    assert dropout_scale(32768) == 2.0 and dropout_scale(49152) == 4.0
    assert dropout_scale(6554) == float(np.float32(65536.0 / (65536 - 6554)))


def test_mask_is_the_documented_formula():
    """dropout_mask against a scalar Python-integer evaluation of the
    contract, at a threshold that splits the lanes."""
    seed, thr, n = 0xDEADBEEFCAFEF00D, 20000, 37
    m = dropout_mask(seed, n, thr)
    assert m.dtype == np.bool_ and m.shape == (n,)
    for i in range(n):
        z = Fo._drop_hash(seed, i >> 2)
        lane = (z >> (16 * (i & 3))) & 0xFFFF
        assert bool(m[i]) == (lane >= thr), i
    assert dropout_mask(seed, n, 0).all()            # thr 0 keeps everything
    assert dropout_mask(seed, 0, thr).shape == (0,)


def test_call_seed_is_the_documented_formula():
    r = DropoutRNG()
    r.seed(42, rank=3)
    r.set_epoch(7)
    r.next_call_seed()
    got = r.next_call_seed()                         # calls == 1
    base = (42 ^ Fo.DROP_SALT ^ (3 * Fo.DROP_RANK_SALT)) & ((1 << 64) - 1)
    assert got == Fo._drop_hash(base, (7 << 32) | 1)
    assert Fo.DROP_SALT & 1 and Fo.DROP_RANK_SALT & 1


# ------------------------------------------------------------- statistics ---

@pytest.mark.parametrize("p", [0.1, 0.5, 0.75])
def test_dropped_count_zscore_cap(p):
    n = 257 * 136
    thr = dropout_threshold(p)
    q = thr / 65536.0
    r = DropoutRNG()
    r.seed(42, rank=0)
    worst = 0.0
    for _ in range(20):
        dropped = n - int(dropout_mask(r.next_call_seed(), n, thr).sum())
        z = (dropped - n * q) / (n * q * (1 - q)) ** 0.5
        worst = max(worst, abs(z))
    print(f"p={p}: worst |z| over 20 calls = {worst:.3f}")
    assert worst <= 4.5


def test_successive_calls_and_ranks_are_independent():
    n, thr = 1 << 20, dropout_threshold(0.5)
    r0, r1 = DropoutRNG(), DropoutRNG()
    r0.seed(42, rank=0)
    r1.seed(42, rank=1)
    a = dropout_mask(r0.next_call_seed(), n, thr)
    b = dropout_mask(r0.next_call_seed(), n, thr)
    c = dropout_mask(r1.next_call_seed(), n, thr)
    succ = float((a == b).mean())
    cross = float((a == c).mean())
    print(f"agreement: successive calls {succ:.4f}, ranks 0/1 {cross:.4f}")
    assert abs(succ - 0.5) <= 0.005
    assert abs(cross - 0.5) <= 0.005


# -------------------------------------------------------------------- rng ---

def test_set_epoch_reproduces_the_sequence():
    r = ops.dropout_rng
    r.set_epoch(3)
    one = [r.next_call_seed() for _ in range(5)]
    r.set_epoch(3)
    two = [r.next_call_seed() for _ in range(5)]
    r.set_epoch(4)
    other = [r.next_call_seed() for _ in range(5)]
    assert one == two and len(set(one)) == 5
    assert not set(one) & set(other)
    assert all(0 <= s < (1 << 64) for s in one)


def test_state_dict_round_trip():
    r = DropoutRNG()
    r.seed(99, rank=2)
    r.set_epoch(5)
    r.next_call_seed()
    sd = r.state_dict()
    ahead = [r.next_call_seed() for _ in range(3)]
    q = DropoutRNG()
    q.load_state_dict(sd)
    assert q.state_dict() == sd
    assert [q.next_call_seed() for _ in range(3)] == ahead


def test_seed_rank_defaults_to_the_process_group_rank_else_zero():
    r = DropoutRNG()
    r.seed(5)
    assert r.rank == (dist.get_rank() if dist.is_initialized() else 0)


# --------------------------------------------------------------- CPU path ---

@pytest.mark.parametrize("p", [0.5, 0.1])
def test_cpu_linear_relu_dropout_matches_float64_formula(p):
    torch.manual_seed(0)
    M, N, K = 9, 7, 5                  # N % 4 != 0: hash groups straddle rows
    lin = ops.modules.Linear(K, N).double()
    drop = ops.Dropout(p)
    x = torch.randn(M, K, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(M, N, dtype=torch.float64)
    ops.dropout_rng.set_epoch(2)
    y = ops.linear_relu_dropout(lin, drop, x)
    y.backward(dy)

    ops.dropout_rng.set_epoch(2)
    seed = ops.dropout_rng.next_call_seed()
    thr = dropout_threshold(p)
    scale = dropout_scale(thr)
    keep = torch.from_numpy(dropout_mask(seed, M * N, thr)).view(M, N)
    assert 0 < int(keep.sum()) < M * N
    w, b = lin.weight.detach(), lin.bias.detach()
    pre = x.detach() @ w.t() + b
    ref = torch.where(keep & (pre > 0), pre * scale, torch.zeros_like(pre))
    dz = torch.where(keep & (pre > 0), dy * scale, torch.zeros_like(dy))
    assert torch.equal(y.detach(), ref)
    torch.testing.assert_close(x.grad, dz @ w, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lin.weight.grad, dz.t() @ x.detach(),
                               rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lin.bias.grad, dz.sum(0),
                               rtol=1e-12, atol=1e-12)


def test_cpu_standalone_dropout_storage_order():
    """Contiguous and channels_last tensors are masked by storage offset."""
    thr = dropout_threshold(0.5)
    x = torch.arange(1, 2 * 10 * 3 * 3 + 1, dtype=torch.float32) \
        .view(2, 10, 3, 3)
    xcl = x.contiguous(memory_format=torch.channels_last)
    for t, flat in ((x, lambda v: v.reshape(-1)),
                    (xcl, lambda v: v.permute(0, 2, 3, 1).reshape(-1))):
        t = t.clone(memory_format=torch.preserve_format).requires_grad_()
        ops.dropout_rng.set_epoch(0)
        y = ops.dropout(t, 0.5, True)
        ops.dropout_rng.set_epoch(0)
        keep = torch.from_numpy(
            dropout_mask(ops.dropout_rng.next_call_seed(), t.numel(), thr))
        assert torch.equal(flat(y.detach()) != 0, keep)
        assert torch.equal(flat(y.detach())[keep], flat(t.detach())[keep] * 2)
        y.sum().backward()
        assert torch.equal(flat(t.grad), keep.float() * 2)


def test_dropout_module_eval_identity_and_refusals():
    d = ops.Dropout(0.5)
    assert isinstance(d, torch.nn.Dropout)
    assert not list(d.parameters()) and not list(d.buffers())
    x = torch.randn(4, 6)
    d.eval()
    before = ops.dropout_rng.state_dict()
    assert d(x) is x
    d.train()
    assert ops.Dropout(0.0)(x) is x
    assert ops.dropout_rng.state_dict() == before    # neither drew a seed
    y = d(x)
    assert y is not x and ops.dropout_rng.calls == before["calls"] + 1
    with pytest.raises(ValueError):
        ops.Dropout(0.5, inplace=True)
    with pytest.raises(ValueError):
        ops.Dropout(1.0)
    with pytest.raises(ValueError):
        ops.Dropout(-0.5)


def test_vgg_dropout_slots_and_default_model():
    from ddp_tricks_amd.models import build_model
    torch.manual_seed(0)
    plain = build_model("vgg16", num_classes=10, cifar_head=True)
    torch.manual_seed(0)
    drop = build_model("vgg16", num_classes=10, cifar_head=True, dropout=0.5)
    for i in (2, 5):
        assert type(plain.classifier[i]) is torch.nn.Dropout
        assert type(drop.classifier[i]) is ops.modules.Dropout
    assert list(plain.state_dict()) == list(drop.state_dict())
    before = ops.dropout_rng.state_dict()
    x = torch.randn(2, 3, 32, 32)
    # same weights, eval mode: the ReLU-only junction equals relu(linear)
    plain.eval()
    drop.eval()
    with torch.no_grad():
        assert torch.equal(plain(x), drop(x))
    assert ops.dropout_rng.state_dict() == before
    # the default model never touches the dropout stream
    plain.train()
    plain(x)
    assert ops.dropout_rng.state_dict() == before
    # training: two junction calls per forward, reproduced by set_epoch
    drop.train()
    ops.dropout_rng.set_epoch(1)
    y1 = drop(x)
    assert ops.dropout_rng.calls == 2
    ops.dropout_rng.set_epoch(1)
    y2 = drop(x)
    assert torch.equal(y1, y2)


# ------------------------------------------------------- run.py plumbing ---

def _load_run():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_dropout", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_flag(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    assert run.parse_args().dropout == 0.0
    monkeypatch.setattr(sys, "argv", ["run.py", "--dropout", "0.5"])
    assert run.parse_args().dropout == 0.5


def _args(tmp_path, **over):
    a = types.SimpleNamespace(
        exp_name="DROP", learning_rate=0.05, batch_size=64, epochs=1,
        warmup_epochs=2, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


class _Stop(Exception):
    pass


@pytest.fixture
def dist_env():
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29641")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("gloo", rank=0, world_size=1)
    yield


def _built_model(tmp_path, monkeypatch, **over):
    """(name, kwargs, model) of train()'s build_model call; training is cut
    right after it."""
    train_mod = importlib.import_module("ddp_tricks_amd.utils.train")
    from ddp_tricks_amd.models import build_model as real
    seen = []

    def spy(name, **kw):
        seen.append((name, kw, real(name, **kw)))
        raise _Stop

    monkeypatch.setattr(train_mod, "build_model", spy)
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "128")
    amp._state.__init__()
    with pytest.raises(_Stop):
        train_mod.train(_args(tmp_path, **over))
    amp._state.__init__()
    return seen[0]


def test_default_run_passes_no_dropout_kwarg(tmp_path, monkeypatch, dist_env):
    name, kw, _ = _built_model(tmp_path, monkeypatch)
    assert name == "toy_net" and "dropout" not in kw
    name, kw, model = _built_model(
        tmp_path, monkeypatch, model="vgg16", dropout=0.0,
        model_kwargs=dict(num_classes=10, cifar_head=True))
    assert "dropout" not in kw
    assert type(model.classifier[2]) is torch.nn.Dropout
    assert ops.dropout_rng.state_dict()["seed"] == 42    # train() keyed it


def test_dropout_flag_builds_hash_dropout_slots(tmp_path, monkeypatch, dist_env):
    small = dict(num_classes=10, cifar_head=True)
    _, kw0, plain = _built_model(tmp_path, monkeypatch, model="vgg16",
                                 model_kwargs=small)
    name, kw, model = _built_model(tmp_path, monkeypatch, model="vgg16",
                                   dropout=0.5, model_kwargs=small)
    assert name == "vgg16" and kw["dropout"] == 0.5
    assert "dropout" not in small                     # caller's dict untouched
    for i in (2, 5):
        assert type(model.classifier[i]) is ops.modules.Dropout
        assert model.classifier[i].p == 0.5
    assert list(model.state_dict()) == list(plain.state_dict())


def test_dropout_flag_refused_for_a_model_without_dropout(tmp_path,
                                                          monkeypatch):
    train_mod = importlib.import_module("ddp_tricks_amd.utils.train")
    with pytest.raises(ValueError, match="dropout"):
        train_mod.train(_args(tmp_path, model="toy_net", dropout=0.5))
    with pytest.raises(ValueError, match="dropout"):
        train_mod.train(_args(tmp_path, model="vgg16", dropout=-0.1))
