"""GPU tier of the device-resident data path: ``ext.batch_gather_aug``
against the CPU reference loader.  The kernel only moves table entries, so
every comparison is ``torch.equal`` — no tolerance anywhere."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

from ddp_tricks_amd.utils.data import (CIFAR10, Augment, DeviceBatchLoader,
                                       FastBatchLoader, reference_batch)

SEED, EPOCH = 42, 3


def _ext():
    from ddp_tricks_amd.ops import load_extension
    return load_extension(required=True)


def _store(n, h, w, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    store = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 1000, (n,), generator=g)
    return store, labels


def _launch(store, labels, index, lut, pad, hflip, seed=SEED, epoch=EPOCH):
    out, lbl = _ext().batch_gather_aug(
        store.to(DEV), labels.to(DEV), index.to(DEV), lut.to(DEV),
        pad, hflip, seed, epoch)
    torch.cuda.synchronize()
    return out, lbl


def _check(store, labels, index, lut, pad, hflip, seed=SEED, epoch=EPOCH):
    out, lbl = _launch(store, labels, index, lut, pad, hflip, seed, epoch)
    N, H, W, C = store.shape
    B = index.numel()
    assert out.dtype == torch.bfloat16 and lbl.dtype == torch.int64
    assert tuple(out.shape) == (B, C, H, W)
    assert out.stride() == (H * W * C, 1, W * C, C)
    assert out.is_contiguous(memory_format=torch.channels_last)
    want = reference_batch(store, lut, index, pad, hflip, seed, epoch)
    assert torch.equal(out.float().cpu(), want)
    assert torch.equal(lbl.cpu(), labels[index.clamp(0, N - 1)])
    return out


class _PosDS:
    """16x16, C = 1, pixel value 16*y + x: every pixel of an image is
    unique, so a wrong dx, dy, flip or pad fill cannot cancel out."""

    def __init__(self, n=11):
        img = (16 * torch.arange(16).view(16, 1)
               + torch.arange(16).view(1, 16)).float() / 255.0
        self.images = img.view(1, 1, 16, 16).repeat(n, 1, 1, 1).contiguous()
        self.labels = torch.arange(n) * 7 % 10

    def __len__(self):
        return self.labels.shape[0]


class _FixedSampler:
    def __init__(self, order, epoch):
        self.order, self.epoch = list(order), epoch

    def __iter__(self):
        return iter(self.order)

    def __len__(self):
        return len(self.order)


def test_position_coded_images():
    ds = _PosDS(11)
    smp = _FixedSampler([0, 10, 4, 10, 7], epoch=2)
    aug = Augment(crop_pad=4, hflip=True)
    (gi, gl), = list(DeviceBatchLoader(ds, 5, sampler=smp, device=DEV,
                                       augment=aug, seed=SEED))
    (ci, cl), = list(DeviceBatchLoader(ds, 5, sampler=smp, augment=aug,
                                       seed=SEED))
    assert gi.dtype == torch.bfloat16 and tuple(gi.shape) == (5, 1, 16, 16)
    assert gi.stride() == (256, 1, 16, 1)
    assert gi.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(gi.float().cpu(), ci)
    assert torch.equal(gl.cpu(), cl) and gl.dtype == torch.int64
    assert torch.equal(gi[1], gi[3])            # the repeated index
    # different dataset indices of the SAME picture get different params
    assert not torch.equal(gi[0], gi[1])


SHAPES = [
    # (N, H, W, C, B)
    (9, 28, 28, 1, 6),      # MNIST row: 28 = 3 vector chunks + 4
    (9, 32, 32, 3, 6),      # CIFAR
    (9, 5, 7, 3, 6),        # odd, non-square, E % 8 != 0: scalar path; P ~ size
    (9, 8, 8, 3, 300),      # many blocks, one wave-tile per sample
    (9, 8, 8, 3, 1),        # B = 1
    (5, 16, 16, 1, 8500),   # > 8192 wave-tiles: the grid-stride loop wraps
    (5, 32, 32, 3, 1500),   # wraps with 6 wave-tiles per sample
]


@pytest.mark.parametrize("pad,hflip", [(0, False), (2, True), (4, True)])
@pytest.mark.parametrize("N,H,W,C,B", SHAPES)
def test_shape_edges(N, H, W, C, B, pad, hflip):
    store, labels = _store(N, H, W, C, seed=H * W + C)
    g = torch.Generator().manual_seed(B)
    index = torch.randint(0, N, (B,), generator=g)
    index[0], index[-1] = 0, N - 1
    _check(store, labels, index, Augment().lut(C), pad, hflip)


def test_lut_normalising_and_random_and_fill():
    store, labels = _store(7, 32, 32, 3, seed=11)
    index = torch.tensor([6, 0, 3, 3, 5])
    norm = Augment(mean=CIFAR10.MEAN, std=CIFAR10.STD).lut(3)
    _check(store, labels, index, norm, 4, True)
    g = torch.Generator().manual_seed(12)
    rnd = torch.randn(3, 256, generator=g).to(torch.bfloat16)
    _check(store, labels, index, rnd, 4, True)
    # pad fill = lut[c][0] per channel: P >= the image size on a store with
    # no zero byte, so every zero the kernel looks up is padding.  Pixels
    # whose source is outside must carry the channel's fill value exactly.
    small = torch.randint(1, 256, (4, 3, 3, 3), dtype=torch.uint8,
                          generator=g)
    idx = torch.arange(4)
    out = _check(small, torch.arange(4), idx, rnd, 4, True).float().cpu()
    no_zero = rnd.clone()
    no_zero[:, 0] = 1000.0                      # move only the fill entry
    moved = _check(small, torch.arange(4), idx, no_zero, 4, True).float().cpu()
    fill = (out != moved)
    assert fill.any() and not fill.all()
    for c in range(3):
        assert torch.all(out[:, c][fill[:, c]] == rnd[c, 0].float())
        assert torch.all(moved[:, c][fill[:, c]] == 1000.0)


def test_index_is_clamped():
    """Documented behaviour: out-of-range indices clamp to [0, N-1] (a host
    range check would cost a device sync per batch)."""
    store, labels = _store(6, 8, 8, 3, seed=13)
    index = torch.tensor([-3, 0, 5, 6, 1 << 40])
    _check(store, labels, index, Augment().lut(3), 2, True)


def test_empty_batch():
    store, labels = _store(3, 8, 8, 3)
    out, lbl = _launch(store, labels, torch.empty(0, dtype=torch.long),
                       Augment().lut(3), 2, True)
    assert tuple(out.shape) == (0, 3, 8, 8) and tuple(lbl.shape) == (0,)


def test_determinism_and_epoch_keying():
    store, labels = _store(64, 32, 32, 3, seed=14)
    index = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    lut = Augment(mean=CIFAR10.MEAN, std=CIFAR10.STD).lut(3)
    a, _ = _launch(store, labels, index, lut, 4, True)
    b, _ = _launch(store, labels, index, lut, 4, True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    c, _ = _launch(store, labels, index, lut, 4, True, epoch=EPOCH + 1)
    assert not torch.equal(a, c)
    d, _ = _launch(store, labels, index, lut, 4, True, seed=SEED + 1)
    assert not torch.equal(a, d)
    # full-width seed / epoch bits reach the hash
    _check(store, labels, index, lut, 4, True, seed=-7, epoch=(1 << 32) - 1)


def test_loader_matches_cpu_loader_over_epochs():
    from ddp_tricks_amd.utils.data import DistributedSampler

    class _DS:
        def __init__(self):
            g = torch.Generator().manual_seed(15)
            self.images = torch.randint(0, 256, (53, 3, 32, 32),
                                        generator=g).float() / 255.0
            self.labels = torch.randint(0, 10, (53,), generator=g)

        def __len__(self):
            return 53

    ds = _DS()
    aug = Augment(crop_pad=4, hflip=True, mean=CIFAR10.MEAN, std=CIFAR10.STD)
    s = DistributedSampler(ds, num_replicas=2, rank=1)
    gpu = DeviceBatchLoader(ds, 8, sampler=s, device=DEV, augment=aug, seed=7)
    cpu = DeviceBatchLoader(ds, 8, sampler=s, augment=aug, seed=7)
    assert len(gpu) == len(cpu) == 4
    for epoch in (0, 5):
        s.set_epoch(epoch)
        got, want = list(gpu), list(cpu)
        assert len(got) == len(want) == 4 and got[-1][0].shape[0] == 3
        for (gi, gl), (ci, cl) in zip(got, want):
            assert torch.equal(gi.float().cpu(), ci)
            assert torch.equal(gl.cpu(), cl)


def test_store_too_large_falls_back(monkeypatch, capsys):
    ds = _PosDS(11)
    monkeypatch.setattr(torch.cuda, "mem_get_info",
                        lambda device=None: (1024, 1 << 30))
    loader = DeviceBatchLoader(ds, 4, device=DEV)
    assert "FastBatchLoader" in capsys.readouterr().out
    batches = list(loader)
    assert len(batches) == len(loader) == 3
    assert batches[0][0].dtype == torch.float32 and batches[0][0].is_cuda
    assert torch.equal(torch.cat([b[0] for b in batches]).cpu(), ds.images)


# ---------------------------------------------------------- end to end ---

class _K255DS:
    def __init__(self, n=128):
        g = torch.Generator().manual_seed(21)
        self.images = torch.randint(0, 256, (n, 1, 28, 28),
                                    generator=g).float() / 255.0
        self.labels = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return self.labels.shape[0]


def _three_steps(make_loader):
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models.toy_net import Toy_Net
    from ddp_tricks_amd.ops.functional import (clear_weight_cache,
                                               cross_entropy_loss)
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.utils.lookahead import Lookahead

    amp._state.__init__()
    clear_weight_cache()
    same_seeds(42)
    model = Toy_Net().to(DEV)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    la = Lookahead(opt, k=10, alpha=0.5)
    model, la = amp.initialize(model, la, opt_level="O1")
    model.train()
    losses = []
    it = iter(make_loader())
    for _ in range(3):
        x, t = next(it)
        la.zero_grad()
        out = model(x)
        loss = cross_entropy_loss(out, t) / out.shape[0]
        with amp.scale_loss(loss, la) as scaled:
            scaled.backward()
        la.step()
        losses.append(float(loss.detach()))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    amp._state.__init__()
    return losses, sd


def test_training_bits_equal_host_path():
    """The stem conv sees identical bf16 bits from either loader and every
    kernel is fixed-order, so 3 steps give equal losses and parameters."""
    ds = _K255DS(128)
    l_host, sd_host = _three_steps(
        lambda: FastBatchLoader(ds, 32, pin_memory=True, device=DEV))
    l_dev, sd_dev = _three_steps(
        lambda: DeviceBatchLoader(ds, 32, device=DEV, augment=Augment()))
    assert l_host == l_dev, (l_host, l_dev)
    for k in sd_host:
        assert torch.equal(sd_host[k], sd_dev[k]), k


def test_train_device_data_flags_gpu(tmp_path, monkeypatch, capsys):
    """train() with --device_data --augment crop_flip --normalize on tiny
    synthetic CIFAR / ResNet-18: 2 epochs, finite losses."""
    import re

    import torch.distributed as dist
    from ddp_tricks_amd import amp
    amp._state.__init__()
    monkeypatch.setenv("DDPX_SYNTH_SAMPLES", "256")
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29678")
        dist.init_process_group("nccl", rank=0, world_size=1)
    from ddp_tricks_amd.utils.train import train
    args = types.SimpleNamespace(
        exp_name="GPU_dd", learning_rate=0.05, batch_size=64, epochs=2,
        warmup_epochs=1, warmup_type="linear", seed_num=42,
        data_path=str(tmp_path / "no_data"), model_path=str(tmp_path),
        local_rank=0, model="resnet18", dataset="cifar10",
        device_data=True, augment="crop_flip", normalize=True)
    try:
        train(args)
    finally:
        amp._state.__init__()
        dist.destroy_process_group()
    out = capsys.readouterr().out
    vals = re.findall(r"(?:train|valid)_loss: (\S+?),", out)
    assert len(vals) == 4, out
    assert all(torch.isfinite(torch.tensor(float(v))) for v in vals), vals
