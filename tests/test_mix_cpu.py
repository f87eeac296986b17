"""Label smoothing and CutMix on the CPU tier: the numpy mirror of the
kernel's mix hash, the reference batch, the soft-target loss, the engine's
handling of a ``MixedTarget`` and the two trainer flags."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from ddp_tricks_amd import amp
from ddp_tricks_amd.ops import MixedTarget, cross_entropy_loss
from ddp_tricks_amd.utils.data import (Augment, DeviceBatchLoader,
                                       DistributedSampler, cutmix_params,
                                       cutmix_threshold, quantize_store,
                                       reference_batch,
                                       reference_batch_cutmix)

_M = (1 << 64) - 1


@pytest.fixture(autouse=True)
def _reset_amp():
    amp._state.__init__()
    yield
    amp._state.__init__()


def _hash(seed, epoch, index):
    key = ((epoch << 32) | index) & _M
    z = (seed + (key + 1) * 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def _py_mix(seed, epoch, index, N, H, W, thresh):
    """The layout of data.hip's header, written with Python ints."""
    z2 = _hash((seed + 0xD1B54A32D192ED03) & _M, epoch, index)
    z3 = _hash((seed + 0x8CB92BA72F3D8DD7) & _M, epoch, index)
    j = ((z2 & 0xFFFFFFFF) * N) >> 32
    r = math.isqrt(z2 >> 32)
    cx = ((z3 & 0xFFFF) * W) >> 16
    cy = (((z3 >> 16) & 0xFFFF) * H) >> 16
    apply = int(((z3 >> 32) & 0xFFFF) < thresh)
    bw, bh = (r * W) >> 16, (r * H) >> 16
    x0, y0 = cx - bw // 2, cy - bh // 2
    box = (max(x0, 0), max(y0, 0), min(x0 + bw, W), min(y0 + bh, H))
    return j, apply, box, (cx, cy, bw, bh)


class _DS:
    """k/255-valued images so the uint8 store round-trips exactly."""

    def __init__(self, n, c, h, w, seed, classes=10):
        g = torch.Generator().manual_seed(seed)
        self.u8 = torch.randint(0, 256, (n, c, h, w), generator=g,
                                dtype=torch.uint8)
        self.images = self.u8.float() / 255.0
        self.labels = torch.randint(0, classes, (n,), generator=g)

    def __len__(self):
        return self.labels.shape[0]


# ------------------------------------------------------------ cutmix_params ---

@pytest.mark.parametrize("seed,epoch,N,H,W", [
    (0, 0, 37, 28, 28), (42, 3, 37, 32, 32), ((1 << 64) - 1, 7, 50000, 5, 7),
    ((1 << 63) + 5, 4294967295, 4294967295, 224, 224), (-3, 1, 1, 1, 1)])
def test_cutmix_params_match_python_ints(seed, epoch, N, H, W):
    idx = np.array([0, 1, 2, 36, 12345, N - 1, 4294967295], dtype=np.int64)
    for prob in (0.0, 0.5, 1.0):
        mp = cutmix_params(seed, epoch, idx, N, H, W, prob)
        for k, i in enumerate(idx.tolist()):
            j, apply, box, raw = _py_mix(seed & _M, epoch, i, N, H, W,
                                         cutmix_threshold(prob))
            assert int(mp.j[k]) == j and int(mp.apply[k]) == apply
            assert tuple(int(b[k]) for b in mp.box) == box
            assert tuple(int(b[k]) for b in mp.raw) == raw


def test_cutmix_params_ranges_area_lam_determinism():
    N, H, W = 37, 28, 32
    idx = np.arange(4000)
    mp = cutmix_params(42, 2, idx, N, H, W, 0.5)
    x0, y0, x1, y1 = mp.box
    cx, cy, bw, bh = mp.raw
    assert mp.j.min() >= 0 and mp.j.max() < N
    assert set(np.unique(mp.apply)) == {0, 1}
    assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
    assert (0 <= cx).all() and (cx < W).all() and (cy < H).all()
    assert (bw <= W).all() and (bh <= H).all() and (bw >= 0).all()
    # a box with a side holds its centre, so clipping never empties it
    full = (bw > 0) & (bh > 0)
    assert ((mp.area > 0) == full).all()
    ys, xs = np.arange(H).reshape(1, H, 1), np.arange(W).reshape(1, 1, W)
    mask = ((xs >= x0.reshape(-1, 1, 1)) & (xs < x1.reshape(-1, 1, 1))
            & (ys >= y0.reshape(-1, 1, 1)) & (ys < y1.reshape(-1, 1, 1)))
    assert (mask.sum((1, 2)) == mp.area).all()
    assert mp.lam.dtype == np.float32
    # HW = 896 < 2^24: lam * HW is an integer recovered exactly in float64
    counted = np.rint(mp.lam.astype(np.float64) * (H * W)).astype(np.int64)
    assert (counted + mp.area * mp.apply == H * W).all()
    assert (mp.lam[mp.apply == 0] == 1.0).all()
    assert (mp.lam == ((H * W - mp.area * mp.apply).astype(np.float32)
                       / np.float32(H * W))).all()
    again = cutmix_params(42, 2, idx[::-1].copy(), N, H, W, 0.5)
    assert (again.j[::-1] == mp.j).all() and (again.area[::-1] == mp.area).all()
    other = cutmix_params(42, 3, idx, N, H, W, 0.5)
    assert (other.j != mp.j).mean() > 0.9
    # prob only moves the apply bit
    p1 = cutmix_params(42, 2, idx, N, H, W, 1.0)
    assert (p1.j == mp.j).all() and (p1.area == mp.area).all()
    assert p1.apply.all() and not cutmix_params(42, 2, idx, N, H, W, 0).apply.any()
    with pytest.raises(ValueError):
        cutmix_threshold(1.5)
    with pytest.raises(ValueError):
        Augment(cutmix_prob=-0.1)


def test_cutmix_distribution():
    """alpha = 1: the unclipped box's area share (r/65536)^2 is uniform, mean
    0.5.  Measured before fixing the figures (seed 42, epoch 0, 20 000
    samples): mean share 0.5007 at 224x224 (the >>16 floors of bw and bh cost
    about 0.67/W: 0.4826 at 32x32), partner decile counts 1958..2050, apply
    rate 0.5029 at prob 0.5."""
    n = 20000
    H = W = 224
    mp = cutmix_params(42, 0, np.arange(n), n, H, W, 0.5)
    cx, cy, bw, bh = mp.raw
    share = (bw * bh) / float(H * W)
    assert abs(share.mean() - 0.5) <= 0.02
    # uniform share: a quarter of the samples in each quarter of [0, 1)
    quart = np.bincount(np.minimum((share * 4).astype(int), 3), minlength=4)
    assert (np.abs(quart - n / 4) < 5 * math.sqrt(n * 3 / 16)).all(), quart
    # partners: 10 bins of expectation 2000, sd 42; 5 sd
    dec = np.bincount(mp.j * 10 // n, minlength=10)
    assert (np.abs(dec - n / 10) < 5 * math.sqrt(n * 0.09)).all(), dec
    assert abs(mp.apply.mean() - 0.5) < 5 * 0.5 / math.sqrt(n)
    for c, size in ((cx, W), (cy, H)):
        assert abs(c.mean() - (size - 1) / 2) < 5 * size / math.sqrt(12 * n)


def test_mix_params_independent_of_batch_and_world():
    ds = _DS(37, 3, 8, 8, seed=3)
    aug = Augment(crop_pad=2, hflip=True, cutmix_prob=0.7)

    def run(num_replicas, rank, batch, epoch):
        s = DistributedSampler(ds, num_replicas=num_replicas, rank=rank)
        s.set_epoch(epoch)
        got = {}
        loader = DeviceBatchLoader(ds, batch, sampler=s, augment=aug, seed=42)
        pos = 0
        order = list(s)
        for im, tg in loader:
            assert isinstance(tg, MixedTarget)
            for k in range(im.shape[0]):
                got[order[pos]] = (im[k], int(tg.a[k]), int(tg.b[k]),
                                   float(tg.lam[k]))
                pos += 1
        return got

    for epoch in (0, 3):
        one = run(1, 0, 8, epoch)
        assert set(one) == set(range(37))
        mp = cutmix_params(42, epoch, np.arange(37), 37, 8, 8, 0.7)
        for rank in (0, 1):
            for i, (im, a, b, lam) in run(2, rank, 5, epoch).items():
                assert torch.equal(im, one[i][0]) and (a, b, lam) == one[i][1:]
                assert a == int(ds.labels[i])
                j = int(mp.j[i]) if mp.apply[i] else i
                assert b == int(ds.labels[j]) and lam == float(mp.lam[i])


def test_reference_batch_cutmix_is_where_of_two_references():
    ds = _DS(37, 3, 6, 9, seed=8)
    store = quantize_store(ds.images)
    lut = Augment().lut(3)
    idx = torch.tensor([0, 5, 36, 99, -4, 5])        # clamped like the kernel
    im, la, lb, lam = reference_batch_cutmix(store, lut, ds.labels, idx, 2,
                                             True, 7, 1, 1.0)
    ic = idx.clamp(0, 36)
    mp = cutmix_params(7, 1, ic.numpy(), 37, 6, 9, 1.0)
    own = reference_batch(store, lut, ic, 2, True, 7, 1)
    oth = reference_batch(store, lut, torch.from_numpy(mp.j), 2, True, 7, 1)
    for k in range(6):
        x0, y0, x1, y1 = (int(b[k]) for b in mp.box)
        want = own[k].clone()
        want[:, y0:y1, x0:x1] = oth[k][:, y0:y1, x0:x1]
        assert torch.equal(im[k], want), k
    assert torch.equal(la, ds.labels[ic])
    assert torch.equal(lb, ds.labels[torch.from_numpy(mp.j)])
    assert torch.equal(lam, torch.from_numpy(mp.lam))
    # prob 0: today's batch, labels twice, lam all ones
    im0, la0, lb0, lam0 = reference_batch_cutmix(store, lut, ds.labels, idx,
                                                 2, True, 7, 1, 0.0)
    assert torch.equal(im0, own) and torch.equal(la0, lb0)
    assert torch.equal(lam0, torch.ones(6))


def test_loader_off_is_todays_call():
    ds = _DS(11, 1, 4, 4, seed=2)
    batches = list(DeviceBatchLoader(ds, 4, augment=Augment(hflip=True)))
    assert all(torch.is_tensor(t) and t.dtype == torch.int64
               for _, t in batches)
    on = list(DeviceBatchLoader(ds, 4, augment=Augment(hflip=True,
                                                       cutmix_prob=1.0)))
    assert all(isinstance(t, MixedTarget) for _, t in on)
    assert [t.a.tolist() for _, t in on] == [t.tolist() for _, t in batches]


# --------------------------------------------------------------------- loss ---

def _closed_form(x, a, b, lam, eps):
    x = x.double()
    B, C = x.shape
    q = torch.full((B, C), eps / C, dtype=torch.float64)
    q += (1 - eps) * (lam.double().view(B, 1) * F.one_hot(a, C)
                      + (1 - lam.double()).view(B, 1) * F.one_hot(b, C))
    assert torch.allclose(q.sum(1), torch.ones(B, dtype=torch.float64))
    return -(q * torch.log_softmax(x, 1)).sum(1).mean()


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_loss_matches_formula_and_closed_form(eps):
    g = torch.Generator().manual_seed(5)
    B, C = 9, 13
    x = torch.randn(B, C, generator=g) * 3
    a = torch.randint(0, C, (B,), generator=g)
    b = torch.randint(0, C, (B,), generator=g)
    b[0] = a[0]
    lam = torch.rand(B, generator=g)
    lam[1], lam[2], lam[3] = 0.0, 1.0, 0.5
    mt = MixedTarget(a, b, lam)
    got = cross_entropy_loss(x, mt, eps)
    ca = F.cross_entropy(x, a, reduction="none", label_smoothing=eps)
    cb = F.cross_entropy(x, b, reduction="none", label_smoothing=eps)
    assert torch.equal(got, (lam * ca + (1 - lam) * cb).mean())
    assert abs(float(got) - float(_closed_form(x, a, b, lam, eps))) < 1e-5
    # a == b: lam drops out, the hard-target (smoothed) loss
    same = cross_entropy_loss(x, MixedTarget(a, a, lam), eps)
    hard = cross_entropy_loss(x, a, eps)
    assert abs(float(same) - float(hard)) < 1e-6
    # (mean of per-row values here, torch's own mean reduction there)
    assert torch.allclose(hard, F.cross_entropy(x, a, label_smoothing=eps),
                          rtol=1e-6, atol=0)
    # defaults: the plain loss, bit for bit
    assert torch.equal(cross_entropy_loss(x, a), F.cross_entropy(x, a))
    # gradient reaches the logits only
    xg = x.clone().requires_grad_(True)
    cross_entropy_loss(xg, mt, eps).backward()
    q = torch.full((B, C), eps / C) + (1 - eps) * (
        lam.view(B, 1) * F.one_hot(a, C) + (1 - lam).view(B, 1)
        * F.one_hot(b, C))
    assert torch.allclose(xg.grad, (torch.softmax(x, 1) - q) / B, atol=1e-6)
    with pytest.raises(ValueError):
        cross_entropy_loss(x, a, 1.0)


def test_mixed_target_to_and_dominant():
    mt = MixedTarget(torch.tensor([1, 2, 3], dtype=torch.int32),
                     torch.tensor([4, 5, 6], dtype=torch.int32),
                     torch.tensor([0.5, 0.49, 1.0], dtype=torch.float64))
    m2 = mt.to(torch.device("cpu"))
    assert m2.a.dtype == m2.b.dtype == torch.int64
    assert m2.lam.dtype == torch.float32 and len(m2) == 3
    assert m2.dominant().tolist() == [1, 5, 3]


# ------------------------------------------------------------------- engine ---

def test_engine_counts_accuracy_on_dominant():
    from ddp_tricks_amd.models.toy_net import Toy_Net
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.utils.engine import iterate_loader
    torch.manual_seed(0)
    ds = _DS(24, 1, 28, 28, seed=9)
    loader = DeviceBatchLoader(ds, 8, augment=Augment(cutmix_prob=1.0),
                               seed=3)
    model = Toy_Net()
    opt = FusedSGD(model.parameters(), lr=0.0, momentum=0.9, nesterov=True)
    model, opt = amp.initialize(model, optimizers=opt, opt_level="O1")
    model.train()
    seen = []

    def loss_fn(out, target):
        assert isinstance(target, MixedTarget)
        seen.append((out.detach().clone(), target))
        return cross_entropy_loss(out, target, 0.1)

    loss, acc, lr = iterate_loader(loader, model, loss_fn, 0, opt,
                                   training=True)
    assert math.isfinite(loss) and lr == 0.0 and len(seen) == 3
    correct = sum(int((o.argmax(1) == t.dominant()).sum()) for o, t in seen)
    assert acc == correct / 24
    doms = torch.cat([t.dominant() for _, t in seen])
    assert not torch.equal(doms, torch.cat([t.a for _, t in seen])), \
        "no sample with lam < 0.5: the case does not tell a from dominant"
    # a tensor target still goes through
    plain = DeviceBatchLoader(ds, 8, augment=Augment(), seed=3)
    model.eval()
    with torch.no_grad():
        loss, acc = iterate_loader(plain, model, cross_entropy_loss, 0, None)
    assert math.isfinite(loss) and 0.0 <= acc <= 1.0


# ---------------------------------------------------------------- trainer ---

def _load_run():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_mix", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_flags(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    a = run.parse_args()
    assert (a.label_smoothing, a.cutmix_prob) == (0.0, 0.0)
    monkeypatch.setattr(sys, "argv", ["run.py", "--label_smoothing", "0.1",
                                      "--cutmix_prob", "0.5"])
    a = run.parse_args()
    assert (a.label_smoothing, a.cutmix_prob) == (0.1, 0.5)


def _args(tmp_path, name, **over):
    a = types.SimpleNamespace(
        exp_name=name, learning_rate=0.1, batch_size=32, epochs=2,
        warmup_epochs=1, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _init_pg(port):
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        dist.init_process_group("gloo", rank=0, world_size=1)


@pytest.mark.timeout(300)
def test_train_both_flags_on(tmp_path, monkeypatch, capsys):
    import ddp_tricks_amd.utils.train  # noqa: F401
    T = sys.modules["ddp_tricks_amd.utils.train"]
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "96")
    built, losses = [], []

    class _SpyDev(DeviceBatchLoader):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)

    real_iter = T.iterate_loader

    def spy_iter(**kw):
        losses.append((kw["training"], kw["loss_function"]))
        return real_iter(**kw)

    monkeypatch.setattr(T, "DeviceBatchLoader", _SpyDev)
    monkeypatch.setattr(T, "iterate_loader", spy_iter)
    _init_pg(29661)
    T.train(_args(tmp_path, "MIX_on", label_smoothing=0.1, cutmix_prob=0.5))
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("epoch:")]
    assert len(lines) == 2 and "nan" not in out
    assert os.path.exists(os.path.join(tmp_path, "MIX_on.pt"))
    tr, va = built        # the flag implies the device loader, train only
    assert tr.augment.cutmix_prob == 0.5 and va.augment.cutmix_prob == 0.0
    assert isinstance(next(iter(tr))[1], MixedTarget)
    assert torch.is_tensor(next(iter(va))[1])
    # smoothing is bound into the training loss; validation keeps the plain one
    for training, fn in losses:
        if training:
            assert fn.func is cross_entropy_loss
            assert fn.keywords == {"label_smoothing": 0.1}
        else:
            assert fn is cross_entropy_loss


@pytest.mark.timeout(300)
def test_train_defaults_unchanged(tmp_path, monkeypatch, capsys):
    """Flags at their defaults: the run of a namespace that does not know
    the flags (what the trainer was called with before they existed)."""
    import ddp_tricks_amd.utils.train  # noqa: F401
    T = sys.modules["ddp_tricks_amd.utils.train"]
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "96")
    losses = []
    real_iter = T.iterate_loader

    def spy_iter(**kw):
        losses.append(kw["loss_function"])
        assert not isinstance(kw["loader"], DeviceBatchLoader)
        return real_iter(**kw)

    monkeypatch.setattr(T, "iterate_loader", spy_iter)
    _init_pg(29662)
    T.train(_args(tmp_path, "MIX_old"))
    amp._state.__init__()
    T.train(_args(tmp_path, "MIX_def", label_smoothing=0.0, cutmix_prob=0.0))
    out = capsys.readouterr().out
    lines = [l.split("time:")[0] + l.split("s, ", 1)[1]
             for l in out.splitlines() if l.startswith("epoch:")]
    assert len(lines) == 4 and lines[:2] == lines[2:]
    assert all(fn is cross_entropy_loss for fn in losses)
    a = torch.load(os.path.join(tmp_path, "MIX_old.pt"))
    b = torch.load(os.path.join(tmp_path, "MIX_def.pt"))
    assert a.keys() == b.keys() and len(a) == 37
    for k in a:
        assert torch.equal(a[k], b[k]), k
