"""Device-resident data path, CPU tier: the augmentation hash (pinned
against literals from a plain Python-int implementation), the CPU reference
loader's semantics and invariances, the FastBatchLoader contract, and the
run.py / train() plumbing of --device_data / --augment / --normalize."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from ddp_tricks_amd import amp
from ddp_tricks_amd.utils import data as D
from ddp_tricks_amd.utils.data import (CIFAR10, MNIST, Augment,
                                       DeviceBatchLoader, DistributedSampler,
                                       FastBatchLoader, SyntheticImageNet,
                                       sample_params)

_M = (1 << 64) - 1


def _py_params(seed, epoch, index, P, hflip=True):
    """The issue's formula, written with Python ints (mod 2^64)."""
    key = ((epoch << 32) | index) & _M
    z = (seed + (key + 1) * 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    z = z ^ (z >> 31)
    dx = ((z & 0xFFFF) * (2 * P + 1)) >> 16
    dy = (((z >> 16) & 0xFFFF) * (2 * P + 1)) >> 16
    return dx, dy, ((z >> 32) & 1) if hflip else 0


# (seed, epoch, index, P) -> (dx, dy, flip); literals computed once with
# _py_params and frozen here: they pin the spec, not the numpy code
HASH_VECTORS = [
    ((0, 0, 0, 4), (7, 4, 1)),
    ((42, 0, 0, 4), (3, 1, 0)),
    ((42, 0, 1, 4), (8, 6, 1)),
    ((42, 1, 0, 4), (8, 4, 1)),
    ((42, 7, 59999, 4), (7, 5, 0)),
    ((1234567, 3, 49999, 2), (2, 2, 1)),
    (((1 << 63) + 5, 4294967295, 4294967295, 4), (1, 2, 1)),
    ((42, 2, 100, 0), (0, 0, 0)),
    (((1 << 64) - 1, 0, 12345, 16), (27, 17, 1)),
]


@pytest.mark.parametrize("args,want", HASH_VECTORS)
def test_hash_vectors(args, want):
    seed, epoch, index, P = args
    assert _py_params(seed, epoch, index, P) == want
    dx, dy, flip = sample_params(seed, epoch, [index], P, True)
    assert (int(dx[0]), int(dy[0]), int(flip[0])) == want
    # hflip off: same offsets, never flipped
    dx, dy, flip = sample_params(seed, epoch, [index], P, False)
    assert (int(dx[0]), int(dy[0]), int(flip[0])) == (want[0], want[1], 0)


def test_hash_distribution():
    """Fixed inputs -> deterministic.  4096 draws over 9 values: binomial
    mean 455, sigma 20.1, so 5 sigma = 100; flips: mean 2048, sigma 32."""
    idx = np.arange(4096)
    dx, dy, flip = sample_params(42, 0, idx, 4, True)
    assert dx.min() >= 0 and dx.max() <= 8 and dy.min() >= 0 and dy.max() <= 8
    cx = np.bincount(dx, minlength=9)
    cy = np.bincount(dy, minlength=9)
    print("dx counts", cx, "dy counts", cy, "flips", int(flip.sum()))
    assert np.all(np.abs(cx - 455) <= 100), cx
    assert np.all(np.abs(cy - 455) <= 100), cy
    assert abs(int(flip.sum()) - 2048) <= 160, int(flip.sum())
    dx1, dy1, flip1 = sample_params(42, 1, idx, 4, True)
    changed = int(((dx != dx1) | (dy != dy1) | (flip != flip1)).sum())
    assert changed > 2048, changed


# ------------------------------------------------------------ fixtures ---

class _DS:
    """Tiny in-memory dataset of k/255 images."""

    def __init__(self, n, c, h, w, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.u8 = torch.randint(0, 256, (n, c, h, w), generator=g,
                                dtype=torch.uint8)
        self.images = self.u8.float() / 255.0
        self.labels = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return self.labels.shape[0]


CIFAR_AUG = dict(crop_pad=4, hflip=True, mean=CIFAR10.MEAN, std=CIFAR10.STD)


def _compose(ds, aug, i, dx, dy, flip):
    """Independent oracle: F.pad + slicing + .flip(-1) on one sample."""
    C, H, W = ds.images.shape[1:]
    P = aug.crop_pad
    lut = aug.lut(C).float()
    padded = F.pad(ds.u8[i].long(), (P, P, P, P))        # zero-pad raw bytes
    crop = padded[:, dy:dy + H, dx:dx + W]
    if flip:
        crop = crop.flip(-1)
    return torch.stack([lut[c][crop[c]] for c in range(C)])


def test_reference_semantics_corner_cases():
    """dx/dy at 0 and 2P, flip on and off — one sample per corner, found
    by scanning the hash over dataset indices."""
    P, n = 4, 4096
    dx, dy, flip = sample_params(5, 3, np.arange(n), P, True)
    ds = _DS(n, 3, 9, 11, seed=1)
    aug = Augment(**CIFAR_AUG)
    picks = []
    for wx in (0, 2 * P):
        for wy in (0, 2 * P):
            for wf in (0, 1):
                hit = np.nonzero((dx == wx) & (dy == wy) & (flip == wf))[0]
                assert hit.size, (wx, wy, wf)
                picks.append(int(hit[0]))
    class _Fixed:
        epoch = 3

        def __iter__(self):
            return iter(picks)

        def __len__(self):
            return len(picks)

    loader = DeviceBatchLoader(ds, 3, sampler=_Fixed(), augment=aug, seed=5)
    got = torch.cat([im for im, _ in loader])
    assert got.dtype == torch.float32 and got.shape == (8, 3, 9, 11)
    for k, i in enumerate(picks):
        want = _compose(ds, aug, i, int(dx[i]), int(dy[i]), int(flip[i]))
        assert torch.equal(got[k], want), (k, i)


def test_reference_all_samples_match_composition():
    ds = _DS(40, 1, 6, 5, seed=2)
    aug = Augment(crop_pad=2, hflip=True)
    dx, dy, flip = sample_params(9, 0, np.arange(40), 2, True)
    loader = DeviceBatchLoader(ds, 16, augment=aug, seed=9)
    got = torch.cat([im for im, _ in loader])
    for i in range(40):
        want = _compose(ds, aug, i, int(dx[i]), int(dy[i]), int(flip[i]))
        assert torch.equal(got[i], want), i


def _by_index(loader, sampler):
    """{dataset index: image} for one epoch of a loader."""
    order = list(sampler)
    imgs = torch.cat([im for im, _ in loader])
    assert imgs.shape[0] == len(order)
    return {i: imgs[k] for k, i in enumerate(order)}


@pytest.mark.parametrize("epoch", [0, 3])
def test_invariance_batch_rank_world_resume(epoch):
    ds = _DS(37, 3, 8, 8, seed=3)
    aug = Augment(**CIFAR_AUG)

    def run(num_replicas, rank, batch):
        s = DistributedSampler(ds, num_replicas=num_replicas, rank=rank)
        s.set_epoch(epoch)
        return _by_index(
            DeviceBatchLoader(ds, batch, sampler=s, augment=aug, seed=42), s)

    one = run(1, 0, 8)
    assert set(one) == set(range(37))
    two = {}
    for rank in (0, 1):
        part = run(2, rank, 4)
        for i, im in part.items():
            assert torch.equal(im, one[i]), (rank, i)
        two.update(part)
    assert set(two) == set(range(37))
    # "resumed": a fresh loader + set_epoch(e) reproduces epoch e, whatever
    # epochs the first loader went through before
    s = DistributedSampler(ds, num_replicas=1, rank=0)
    loader = DeviceBatchLoader(ds, 8, sampler=s, augment=aug, seed=42)
    for e in range(epoch + 1):
        s.set_epoch(e)
        last = _by_index(loader, s)
    for i in one:
        assert torch.equal(last[i], one[i]), i
    if epoch:
        s.set_epoch(0)
        other = _by_index(loader, s)
        assert sum(not torch.equal(other[i], one[i]) for i in one) > 18


def test_contract_matches_fast_batch_loader():
    ds = _DS(37, 1, 7, 6, seed=4)
    # 37 samples over 2 replicas pads one repeated index in; batch 5 leaves
    # a partial last batch (19 = 3*5 + 4)
    for num_replicas, rank in ((1, 0), (2, 1)):
        s = DistributedSampler(ds, num_replicas=num_replicas, rank=rank)
        s.set_epoch(2)
        fast = list(FastBatchLoader(ds, 5, sampler=s))
        loader = DeviceBatchLoader(ds, 5, sampler=s, augment=Augment())
        dev = list(loader)
        assert len(dev) == len(fast) == len(loader)
        assert dev[-1][0].shape[0] == len(s) % 5
        for (di, dl), (fi, fl) in zip(dev, fast):
            assert torch.equal(dl, fl) and dl.dtype == torch.int64
            assert torch.equal(di, fi.to(torch.bfloat16).float())
    # no sampler: sequential order
    fast = list(FastBatchLoader(ds, 16))
    dev = list(DeviceBatchLoader(ds, 16))
    assert [d[1].tolist() for d in dev] == [f[1].tolist() for f in fast]
    assert torch.equal(torch.cat([d[0] for d in dev]),
                       ds.images.to(torch.bfloat16).float())


def test_repeated_indices():
    ds = _DS(5, 3, 4, 4, seed=5)

    class _Rep:
        epoch = 1

        def __iter__(self):
            return iter([4, 0, 4, 4, 2, 0])

        def __len__(self):
            return 6

    aug = Augment(crop_pad=1, hflip=True)
    im, lb = next(iter(DeviceBatchLoader(ds, 6, sampler=_Rep(), augment=aug)))
    assert lb.tolist() == ds.labels[[4, 0, 4, 4, 2, 0]].tolist()
    assert torch.equal(im[0], im[2]) and torch.equal(im[0], im[3])
    assert torch.equal(im[1], im[5])


def test_lut_and_dataset_constants():
    t = Augment().lut(3)
    assert t.shape == (3, 256) and t.dtype == torch.bfloat16
    want = (torch.arange(256, dtype=torch.float32) / 255).to(torch.bfloat16)
    assert all(torch.equal(t[c], want) for c in range(3))
    t = Augment(mean=CIFAR10.MEAN, std=CIFAR10.STD).lut(3)
    u = torch.arange(256, dtype=torch.float32) / 255
    for c in range(3):
        assert torch.equal(
            t[c], ((u - CIFAR10.MEAN[c]) / CIFAR10.STD[c]).to(torch.bfloat16))
    with pytest.raises(ValueError):
        Augment(mean=MNIST.MEAN, std=MNIST.STD).lut(3)
    with pytest.raises(ValueError):
        Augment(mean=(0.5,))
    for cls, c in ((MNIST, 1), (CIFAR10, 3), (SyntheticImageNet, 3)):
        assert len(cls.MEAN) == len(cls.STD) == c
        assert all(0 < m < 1 for m in cls.MEAN) and all(s > 0 for s in cls.STD)


def test_quantize_store_roundtrip():
    ds = _DS(9, 3, 4, 5, seed=6)
    store = D.quantize_store(ds.images, chunk=4)
    assert store.dtype == torch.uint8 and store.shape == (9, 4, 5, 3)
    assert torch.equal(store.permute(0, 3, 1, 2), ds.u8)


# ------------------------------------------------------------------ CLI ---

def _load_run():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_dd", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_flags(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    a = run.parse_args()
    assert (a.device_data, a.augment, a.normalize) == (False, "none", False)
    monkeypatch.setattr(sys, "argv", ["run.py", "--device_data", "--augment",
                                      "crop_flip", "--normalize"])
    a = run.parse_args()
    assert (a.device_data, a.augment, a.normalize) == (True, "crop_flip", True)
    monkeypatch.setattr(sys, "argv", ["run.py", "--augment", "bogus"])
    with pytest.raises(SystemExit):
        run.parse_args()


def _train_args(tmp_path, name, **over):
    a = types.SimpleNamespace(
        exp_name=name, learning_rate=0.05, batch_size=16, epochs=2,
        warmup_epochs=1, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0, model="resnet18", dataset="cifar10")
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.timeout(300)
def test_train_cli_flags_cpu(tmp_path, monkeypatch, capsys):
    """2-epoch CPU train() with --augment crop_flip --normalize runs the
    reference path end to end; without the flags the loaders are today's."""
    import ddp_tricks_amd.utils.train  # noqa: F401
    # the package re-exports the train() function under the module's name
    T = sys.modules["ddp_tricks_amd.utils.train"]
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "32")
    built = []

    class _SpyDev(DeviceBatchLoader):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)

    class _SpyFast(FastBatchLoader):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)

    monkeypatch.setattr(T, "DeviceBatchLoader", _SpyDev)
    monkeypatch.setattr(T, "FastBatchLoader", _SpyFast)
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29658")
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        amp._state.__init__()
        T.train(_train_args(tmp_path, "DD_on", augment="crop_flip",
                            normalize=True))
        out = capsys.readouterr().out
        assert len([l for l in out.splitlines()
                    if l.startswith("epoch:")]) == 2
        assert "nan" not in out
        assert os.path.exists(os.path.join(tmp_path, "DD_on.pt"))
        assert [type(b) for b in built] == [_SpyDev, _SpyDev]
        tr, va = built
        assert (tr.augment.crop_pad, tr.augment.hflip) == (4, True)
        assert tr.augment.mean == CIFAR10.MEAN and tr.seed == 42
        assert (va.augment.crop_pad, va.augment.hflip) == (0, False)
        assert va.augment.std == CIFAR10.STD and va.sampler is None

        del built[:]
        amp._state.__init__()
        T.train(_train_args(tmp_path, "DD_off"))
        assert [type(b) for b in built] == [_SpyFast, _SpyFast]
        assert os.path.exists(os.path.join(tmp_path, "DD_off.pt"))
    finally:
        amp._state.__init__()
        dist.destroy_process_group()
