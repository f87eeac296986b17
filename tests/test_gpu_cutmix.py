"""GPU tier of CutMix in the batch kernel: ``ext.batch_gather_cutmix``
against ``reference_batch_cutmix``.  The kernel only moves table entries and
its parameters are integers (lam is one correctly rounded fp32 division), so
every comparison is ``torch.equal`` — images, labels_a, labels_b and lam."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

from ddp_tricks_amd.utils.data import (Augment, DeviceBatchLoader,
                                       cutmix_params, cutmix_threshold,
                                       reference_batch_cutmix)

N = 37
EPOCHS = (3, 4)
# (H, W, C) -> seed, found on the CPU with cutmix_params so that indices
# 0..36 over the two epochs hold every case of _coverage (asserted below)
SHAPES = {
    (28, 28, 1): 4,       # VEC = 8
    (32, 32, 3): 4,       # VEC = 8, chunks straddle pixels and box edges
    (5, 7, 3): 1,         # E = 105: VEC = 1
}
SHAPE_IDS = ["28x28x1", "32x32x3", "5x7x3"]


def _ext():
    from ddp_tricks_amd.ops import load_extension
    return load_extension(required=True)


def _store(h, w, c):
    g = torch.Generator().manual_seed(h * w + c)
    store = torch.randint(0, 256, (N, h, w, c), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 1000, (N,), generator=g)
    return store, labels


def _coverage(seed, H, W, C):
    """case name -> [(epoch, index), ...] over indices 0..N-1, EPOCHS"""
    got = {k: [] for k in ("empty", "left", "right", "top", "bottom", "half",
                           "self", "not_applied", "applied", "edge_in_chunk")}
    idx = np.arange(N)
    for ep in EPOCHS:
        mp = cutmix_params(seed, ep, idx, N, H, W, 1.0)
        ap = cutmix_params(seed, ep, idx, N, H, W, 0.5).apply
        cx, cy, bw, bh = mp.raw
        x0, y0, x1, y1 = mp.box
        full = (bw > 0) & (bh > 0)
        flags = {
            "empty": ~full,
            "left": full & (cx - bw // 2 < 0),
            "right": full & (cx - bw // 2 + bw > W),
            "top": full & (cy - bh // 2 < 0),
            "bottom": full & (cy - bh // 2 + bh > H),
            "half": 2 * mp.area >= H * W,
            "self": mp.j == idx,
            "not_applied": ap == 0,
            "applied": ap == 1,
        }
        # a left or right box edge strictly inside a 16-byte (8-element) chunk
        edge = np.zeros(N, dtype=bool)
        for k in range(N):
            for xe in (int(x0[k]), int(x1[k])):
                if mp.area[k] and 0 < xe < W:
                    edge[k] |= any(((y * W + xe) * C) % 8
                                   for y in range(int(y0[k]), int(y1[k])))
        flags["edge_in_chunk"] = edge
        for name, f in flags.items():
            got[name] += [(ep, int(i)) for i in idx[f]]
    return got


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_chosen_seeds_cover_every_case(shape):
    H, W, C = shape
    cov = _coverage(SHAPES[shape], H, W, C)
    for name, hits in cov.items():
        if name == "edge_in_chunk" and (H * W * C) % 8:
            continue                      # VEC = 1: a chunk is one element
        assert hits, (shape, name)


def _index(B, shape):
    """B = 70: every index, out-of-range ones (clamped to 0 and N-1) and
    repeats; B = 5 and B = 1: indices of named cases."""
    H, W, C = shape
    if B == 70:
        extra = [-5, N, 1000, -1] + [(7 * k) % N for k in range(29)]
        return torch.tensor(list(range(N)) + extra)
    cov = _coverage(SHAPES[shape], H, W, C)
    picks = [cov[name][0][1] for name in ("edge_in_chunk", "empty", "self",
                                          "half", "left")
             if cov[name]]
    picks += list(range(5))
    return torch.tensor(picks[:B])


def _launch(store, labels, index, lut, pad, hflip, seed, epoch, prob):
    out = _ext().batch_gather_cutmix(
        store.to(DEV), labels.to(DEV), index.to(DEV), lut.to(DEV), pad, hflip,
        seed, epoch, cutmix_threshold(prob))
    torch.cuda.synchronize()
    return out


def _check(store, labels, index, lut, pad, hflip, seed, epoch, prob):
    im, la, lb, lam = _launch(store, labels, index, lut, pad, hflip, seed,
                              epoch, prob)
    _, H, W, C = store.shape
    B = index.numel()
    assert im.dtype == torch.bfloat16 and tuple(im.shape) == (B, C, H, W)
    assert im.is_contiguous(memory_format=torch.channels_last)
    assert la.dtype == lb.dtype == torch.int64 and lam.dtype == torch.float32
    assert la.shape == lb.shape == lam.shape == (B,)
    wi, wa, wb, wl = reference_batch_cutmix(store, lut, labels, index, pad,
                                            hflip, seed, epoch, prob)
    assert torch.equal(la.cpu(), wa) and torch.equal(lb.cpu(), wb)
    assert torch.equal(lam.cpu(), wl)
    got = im.float().cpu()
    assert torch.equal(got, wi), (got != wi).flatten(1).sum(1).tolist()
    return im, la, lb, lam


@pytest.mark.parametrize("prob", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_matches_reference(shape, B, pad, prob):
    H, W, C = shape
    store, labels = _store(H, W, C)
    index = _index(B, shape)
    lut = Augment().lut(C)
    for epoch in EPOCHS:
        im, la, lb, lam = _check(store, labels, index, lut, pad, True,
                                 SHAPES[shape], epoch, prob)
        if prob == 0.0:
            assert torch.equal(la, lb)
            assert torch.equal(lam, torch.ones_like(lam))
    if B == 70:     # out-of-range indices are clamped as before
        assert la[N:N + 4].tolist() == labels[[0, N - 1, N - 1, 0]].tolist()


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_prob_zero_is_batch_gather_aug(shape):
    H, W, C = shape
    store, labels = _store(H, W, C)
    index = _index(70, shape)
    lut = Augment(mean=(0.5,) * C, std=(0.25,) * C).lut(C)
    args = (store.to(DEV), labels.to(DEV), index.to(DEV), lut.to(DEV), 4,
            True, SHAPES[shape], EPOCHS[0])
    im0, l0 = _ext().batch_gather_aug(*args)
    im, la, lb, lam = _ext().batch_gather_cutmix(*args, 0)
    assert torch.equal(im, im0) and im.stride() == im0.stride()
    assert torch.equal(la, l0) and torch.equal(lb, l0)
    assert torch.equal(lam, torch.ones(70, device=DEV))


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_row_does_not_depend_on_the_batch(shape):
    H, W, C = shape
    store, labels = _store(H, W, C)
    lut = Augment().lut(C)
    index = _index(70, shape)
    seed = SHAPES[shape]
    big = _launch(store, labels, index, lut, 4, True, seed, EPOCHS[1], 1.0)
    cov = _coverage(seed, H, W, C)
    rows = {cov[name][-1][1] for name in cov if cov[name]} | {0, N - 1}
    for i in sorted(rows):
        one = _launch(store, labels, index[i:i + 1], lut, 4, True, seed,
                      EPOCHS[1], 1.0)
        for o, b in zip(one, big):
            assert torch.equal(o[0], b[i]), i


def test_lam_is_the_rounded_quotient():
    """Every area 0..HW of a 5x7 image occurs as (HW - area)/HW somewhere in
    a large draw; the kernel's lam equals numpy's float32 quotient."""
    H, W, C = 5, 7, 3
    store, labels = _store(H, W, C)
    lut = Augment().lut(C)
    index = torch.arange(N).repeat(2)
    seen = set()
    for seed in range(8):
        _, _, _, lam = _check(store, labels, index, lut, 0, False, seed, 0,
                              1.0)
        seen |= set(lam.cpu().tolist())
    assert len(seen) >= 12, sorted(seen)


class _DS:
    def __init__(self, store, labels):
        self.images = store.permute(0, 3, 1, 2).float() / 255.0
        self.labels = labels

    def __len__(self):
        return self.labels.shape[0]


def test_loader_yields_mixed_targets():
    from ddp_tricks_amd.ops import MixedTarget
    store, labels = _store(32, 32, 3)
    ds = _DS(store, labels)
    aug = Augment(crop_pad=4, hflip=True, cutmix_prob=0.5)
    gpu = list(DeviceBatchLoader(ds, 16, device=DEV, augment=aug, seed=4))
    cpu = list(DeviceBatchLoader(ds, 16, augment=aug, seed=4))
    assert len(gpu) == len(cpu) == 3
    for (gi, gt), (ci, ct) in zip(gpu, cpu):
        assert isinstance(gt, MixedTarget) and gt.a.is_cuda
        assert torch.equal(gi.float().cpu(), ci)
        assert torch.equal(gt.a.cpu(), ct.a) and torch.equal(gt.b.cpu(), ct.b)
        assert torch.equal(gt.lam.cpu(), ct.lam)
    # CutMix off: the loader's batches are what they were, tensor labels
    off = list(DeviceBatchLoader(ds, 16, device=DEV,
                                 augment=Augment(crop_pad=4, hflip=True),
                                 seed=4))
    assert all(torch.is_tensor(t) for _, t in off)


def test_host_checks():
    store, labels = _store(5, 7, 3)
    lut = Augment().lut(3)
    args = (store.to(DEV), labels.to(DEV), torch.arange(4, device=DEV),
            lut.to(DEV), 0, False, 1, 0)
    for thresh in (-1, 65537):
        with pytest.raises(RuntimeError):
            _ext().batch_gather_cutmix(*args, thresh)
    with pytest.raises(RuntimeError):
        _ext().batch_gather_cutmix(args[0], args[1], torch.arange(4),
                                   *args[3:], 100)
    im, la, lb, lam = _ext().batch_gather_cutmix(
        args[0], args[1], torch.zeros(0, dtype=torch.long, device=DEV),
        *args[3:], 100)
    assert im.shape[0] == la.numel() == lb.numel() == lam.numel() == 0
