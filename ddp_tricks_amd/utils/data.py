"""Data pipeline: MNIST IDX reader, synthetic fallback, DistributedSampler,
and a CUDA prefetching loader wrapper.

Replaces the reference's torchvision.MNIST + torch DistributedSampler +
pin_memory DataLoader stack (reference utils/train.py:24-30) without
torchvision and without network access:

  * ``MNIST`` reads the raw IDX (optionally gzipped) files if present under
    ``{root}/MNIST/raw`` and otherwise builds a deterministic synthetic
    look-alike (60k/10k × 1×28×28, 10 classes, class-dependent patterns) so
    every pipeline above it behaves identically.
  * ``DistributedSampler`` matches torch's semantics: per-epoch seeded
    shuffle, padding to a rank-divisible length, ``set_epoch``.
  * ``CudaPrefetcher`` stages batches pinned and copies H2D on a dedicated
    copy stream one batch ahead (SURVEY N15 disposition).
  * ``DeviceBatchLoader`` (opt-in) keeps the dataset on the GPU as uint8 and
    builds each batch — gather, crop, flip, normalise, bf16 channels_last —
    with one HIP kernel launch (``ops/hip/data.hip``); on CPU it is the
    reference implementation of the same augmentation.  With
    ``Augment(cutmix_prob=...)`` the same launch also pastes a hashed box of
    a partner sample (CutMix) and the batches carry ``MixedTarget`` labels.
"""
from __future__ import annotations

import collections
import gzip
import math
import os
import struct
from typing import Iterator, Optional

import numpy as np
import torch
from torch.utils.data import Dataset


def _read_idx(path: str) -> np.ndarray:
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        magic = struct.unpack(">I", f.read(4))[0]
        ndim = magic & 0xFF
        dims = [struct.unpack(">I", f.read(4))[0] for _ in range(ndim)]
        data = np.frombuffer(f.read(), dtype=np.uint8)
    return data.reshape(dims)


def _find_idx(root: str, base: str) -> Optional[str]:
    for sub in ("MNIST/raw", "MNIST", "raw", "."):
        for ext in ("", ".gz"):
            p = os.path.join(root, sub, base + ext)
            if os.path.exists(p):
                return p
    return None


def _offline() -> bool:
    return os.environ.get("DDPX_OFFLINE", "0") == "1"


_MNIST_MIRRORS = (
    "https://ossci-datasets.s3.amazonaws.com/mnist/",
    "http://yann.lecun.com/exdb/mnist/",
)


def _download_mnist(root: str, bases) -> None:
    """Best-effort fetch of the raw IDX .gz files (reference parity:
    torchvision download=True at reference utils/train.py:25).  In the
    offline build/test environment this fails fast and the caller falls
    back to local files / synthetic data.  DDPX_OFFLINE=1 skips the attempt
    (and the directory it would create) altogether — the test suite sets it."""
    if _offline():
        return
    import urllib.error
    import urllib.request
    dest = os.path.join(root, "MNIST", "raw")
    os.makedirs(dest, exist_ok=True)
    for base in bases:
        fname = base + ".gz"
        out = os.path.join(dest, fname)
        if os.path.exists(out) or os.path.exists(out[:-3]):
            continue
        for mirror in _MNIST_MIRRORS:
            try:
                with urllib.request.urlopen(mirror + fname, timeout=15) as r, \
                        open(out + ".part", "wb") as f:
                    while True:
                        chunk = r.read(1 << 20)
                        if not chunk:
                            break
                        f.write(chunk)
                os.replace(out + ".part", out)
                break
            except (urllib.error.URLError, OSError, ValueError):
                continue
        else:
            import warnings
            warnings.warn(f"MNIST download failed for {fname} "
                          "(no network?); falling back to local/synthetic")


class MNIST(Dataset):
    """MNIST (or a deterministic synthetic stand-in when files are absent).

    Returns (float32 [1,28,28] in [0,1], int64 label) like
    torchvision.MNIST with ToTensor (reference utils/train.py:25).
    """

    # usual published constants; read only when normalisation is requested
    MEAN = (0.1307,)
    STD = (0.3081,)

    def __init__(self, root: str = "./datasets/", train: bool = True,
                 download: bool = False, synthetic: Optional[bool] = None,
                 num_samples: Optional[int] = None):
        base_img = "train-images-idx3-ubyte" if train else "t10k-images-idx3-ubyte"
        base_lbl = "train-labels-idx1-ubyte" if train else "t10k-labels-idx1-ubyte"
        img_path = _find_idx(root, base_img)
        lbl_path = _find_idx(root, base_lbl)
        if download and not (img_path and lbl_path) and synthetic is not True:
            _download_mnist(root, (base_img, base_lbl))
            img_path = _find_idx(root, base_img)
            lbl_path = _find_idx(root, base_lbl)
        n_default = 60000 if train else 10000
        self.synthetic = synthetic if synthetic is not None else not (img_path and lbl_path)
        if not self.synthetic:
            images = _read_idx(img_path).astype(np.float32) / 255.0
            labels = _read_idx(lbl_path).astype(np.int64)
            self.images = torch.from_numpy(images).unsqueeze(1).contiguous()
            self.labels = torch.from_numpy(labels)
        else:
            env_cap = os.environ.get("DDPX_SYNTH_SAMPLES")
            if num_samples is None and env_cap:
                num_samples = min(int(env_cap), n_default)
            n = num_samples or n_default
            # Class templates come from a FIXED seed shared by train and
            # valid (a validation set drawn from different class patterns
            # is unlearnable); labels/noise differ per split.
            gt = torch.Generator().manual_seed(9999)
            templates = torch.rand(10, 1, 28, 28, generator=gt)
            g = torch.Generator().manual_seed(1234 if train else 4321)
            labels = torch.randint(0, 10, (n,), generator=g)
            noise = torch.rand(n, 1, 28, 28, generator=g)
            self.images = (0.6 * templates[labels] + 0.4 * noise).clamp_(0, 1)
            self.labels = labels

    def __len__(self) -> int:
        return self.labels.shape[0]

    def __getitem__(self, idx: int):
        return self.images[idx], int(self.labels[idx])


class CIFAR10(Dataset):
    """CIFAR-10 (synthetic stand-in when the binary batches are absent —
    no network in this environment).  Returns (float32 [3,32,32] in [0,1],
    int64 label); BASELINE.json config 4."""

    MEAN = (0.4914, 0.4822, 0.4465)
    STD = (0.2470, 0.2435, 0.2616)

    @staticmethod
    def _download(root: str) -> None:
        """Best-effort fetch+extract of the python-batches tarball
        (torchvision download=True parity; offline → warn and fall back)."""
        if _offline():
            return
        import tarfile
        import urllib.error
        import urllib.request
        url = ("https://www.cs.toronto.edu/~kriz/cifar-10-python.tar.gz")
        os.makedirs(root, exist_ok=True)
        tgz = os.path.join(root, "cifar-10-python.tar.gz")
        try:
            with urllib.request.urlopen(url, timeout=20) as r, \
                    open(tgz + ".part", "wb") as f:
                while True:
                    chunk = r.read(1 << 20)
                    if not chunk:
                        break
                    f.write(chunk)
            os.replace(tgz + ".part", tgz)
            with tarfile.open(tgz, "r:gz") as tf:
                tf.extractall(root)
        except (urllib.error.URLError, OSError, ValueError, tarfile.TarError):
            import warnings
            warnings.warn("CIFAR-10 download failed (no network?); "
                          "falling back to local/synthetic")

    def __init__(self, root: str = "./datasets/", train: bool = True,
                 download: bool = False, synthetic: Optional[bool] = None,
                 num_samples: Optional[int] = None):
        batch_dir = os.path.join(root, "cifar-10-batches-py")
        if download and not os.path.isdir(batch_dir) and synthetic is not True:
            self._download(root)
        self.synthetic = synthetic if synthetic is not None \
            else not os.path.isdir(batch_dir)
        n_default = 50000 if train else 10000
        if not self.synthetic:
            import pickle
            names = [f"data_batch_{i}" for i in range(1, 6)] if train \
                else ["test_batch"]
            imgs, lbls = [], []
            for nm in names:
                with open(os.path.join(batch_dir, nm), "rb") as f:
                    d = pickle.load(f, encoding="bytes")
                imgs.append(np.asarray(d[b"data"], dtype=np.float32) / 255.0)
                lbls.extend(d[b"labels"])
            self.images = torch.from_numpy(
                np.concatenate(imgs).reshape(-1, 3, 32, 32))
            self.labels = torch.tensor(lbls, dtype=torch.int64)
        else:
            env_cap = os.environ.get("DDPX_SYNTH_SAMPLES")
            if num_samples is None and env_cap:
                num_samples = min(int(env_cap), n_default)
            n = num_samples or n_default
            gt = torch.Generator().manual_seed(8888)   # shared templates
            templates = torch.rand(10, 3, 32, 32, generator=gt)
            g = torch.Generator().manual_seed(777 if train else 778)
            labels = torch.randint(0, 10, (n,), generator=g)
            noise = torch.rand(n, 3, 32, 32, generator=g)
            self.images = (0.6 * templates[labels] + 0.4 * noise).clamp_(0, 1)
            self.labels = labels

    def __len__(self) -> int:
        return self.labels.shape[0]

    def __getitem__(self, idx: int):
        return self.images[idx], int(self.labels[idx])


class SyntheticImageNet(Dataset):
    """Synthetic ImageNet-shaped data ([3,224,224], 1000 classes) for the
    ResNet-50 config (BASELINE.json config 5).  Class identity comes from a
    shared 14x14 patch bank tiled up to 224x224 (learnable; full-res
    templates would be 600 MB); images are materialized VECTORIZED in
    __init__ (per-item generation measured seconds-slow) so the in-memory
    FastBatchLoader path applies.  Size defaults are modest — host RAM is
    ~600 KB/image fp32."""

    MEAN = (0.485, 0.456, 0.406)
    STD = (0.229, 0.224, 0.225)

    def __init__(self, root: str = "./datasets/", train: bool = True,
                 download: bool = False, num_samples: Optional[int] = None):
        n_default = 4096 if train else 1024
        env_cap = os.environ.get("DDPX_SYNTH_SAMPLES")
        if num_samples is None and env_cap:
            num_samples = min(int(env_cap), n_default)
        n = num_samples or n_default
        gt = torch.Generator().manual_seed(55555)      # shared patch bank
        patches = torch.rand(1000, 3, 14, 14, generator=gt)
        g = torch.Generator().manual_seed(606 if train else 607)
        self.labels = torch.randint(0, 1000, (n,), generator=g)
        base = patches[self.labels]
        base = base.repeat_interleave(16, 2).repeat_interleave(16, 3)
        noise = torch.rand(n, 3, 224, 224, generator=g)
        self.images = (0.6 * base + 0.4 * noise).clamp_(0, 1)

    def __len__(self) -> int:
        return self.labels.shape[0]

    def __getitem__(self, idx: int):
        return self.images[idx], int(self.labels[idx])


DATASETS = {"mnist": MNIST, "cifar10": CIFAR10,
            "imagenet_synthetic": SyntheticImageNet}


class DistributedSampler(torch.utils.data.Sampler):
    """torch.utils.data.distributed.DistributedSampler semantics
    (seeded shuffle, pad to divisible, set_epoch) re-implemented."""

    def __init__(self, dataset, num_replicas: Optional[int] = None,
                 rank: Optional[int] = None, shuffle: bool = True,
                 seed: int = 0, drop_last: bool = False):
        import torch.distributed as dist
        if num_replicas is None:
            num_replicas = dist.get_world_size() if dist.is_initialized() else 1
        if rank is None:
            rank = dist.get_rank() if dist.is_initialized() else 0
        self.dataset = dataset
        self.num_replicas = num_replicas
        self.rank = rank
        self.epoch = 0
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        n = len(dataset)
        if drop_last and n % num_replicas:
            self.num_samples = n // num_replicas
        else:
            self.num_samples = math.ceil(n / num_replicas)
        self.total_size = self.num_samples * num_replicas

    def __iter__(self) -> Iterator[int]:
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        if not self.drop_last:
            padding = self.total_size - len(indices)
            if padding > 0:
                indices += (indices * math.ceil(padding / max(len(indices), 1)))[:padding]
        else:
            indices = indices[: self.total_size]
        indices = indices[self.rank: self.total_size: self.num_replicas]
        assert len(indices) == self.num_samples
        return iter(indices)

    def __len__(self) -> int:
        return self.num_samples

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch


class CudaPrefetcher:
    """Wrap a DataLoader: pinned H2D copies one batch ahead on a copy stream."""

    def __init__(self, loader, device: torch.device):
        self.loader = loader
        self.device = device
        self.stream = torch.cuda.Stream(device=device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        it = iter(self.loader)
        next_batch = None

        def _preload():
            nonlocal next_batch
            try:
                image, target = next(it)
            except StopIteration:
                next_batch = None
                return
            with torch.cuda.stream(self.stream):
                next_batch = (
                    image.to(self.device, non_blocking=True),
                    target.to(self.device, non_blocking=True),
                )

        _preload()
        while next_batch is not None:
            main = torch.cuda.current_stream(self.device)
            main.wait_stream(self.stream)
            batch = next_batch
            # tensors were allocated on the copy stream; mark their use on
            # the main stream so the caching allocator doesn't recycle them
            # under in-flight kernels (torch stream-semantics rule)
            batch[0].record_stream(main)
            batch[1].record_stream(main)
            _preload()
            yield batch


class FastBatchLoader:
    """Vectorized batch loader for in-memory tensor datasets (MNIST/CIFAR):
    one ``index_select`` per batch instead of per-item ``__getitem__`` +
    collation — the Python loader was the epoch wall-time bound once the
    GPU step dropped to ~3.7 ms.  Preserves DataLoader semantics: iterates
    (images, labels) batches in the order produced by ``sampler`` (or
    sequentially when sampler is None), honors ``set_epoch`` through the
    sampler, optional pinned-memory staging for async H2D.
    """

    SLOTS = 4   # pinned-staging rotation depth (per-slot event guards reuse)

    def __init__(self, dataset, batch_size: int, sampler=None,
                 pin_memory: bool = False, device=None):
        self.dataset = dataset
        self.batch_size = batch_size
        self.sampler = sampler
        self.device = device
        self.gpu = (device is not None and device.type == "cuda"
                    and torch.cuda.is_available())
        self.pin = pin_memory and self.gpu

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        if self.sampler is not None:
            idx = torch.as_tensor(list(self.sampler), dtype=torch.long)
        else:
            idx = torch.arange(len(self.dataset), dtype=torch.long)
        images = self.dataset.images
        labels = self.dataset.labels
        B = self.batch_size
        if not self.gpu:
            for s0 in range(0, idx.numel(), B):
                sel = idx[s0:s0 + B]
                yield (torch.index_select(images, 0, sel),
                       torch.index_select(labels, 0, sel))
            return
        if not self.pin:
            # pin_memory=False honored: plain pageable H2D,
            # no staging buffers, synchronous copy semantics.
            for s0 in range(0, idx.numel(), B):
                sel = idx[s0:s0 + B]
                yield (torch.index_select(images, 0, sel).to(self.device),
                       torch.index_select(labels, 0, sel).to(self.device))
            return
        # GPU path: own the pinned staging AND the H2D (one-ahead on a copy
        # stream).  Slot reuse is guarded by a host event-sync: the host can
        # run many steps ahead of the device, so "old enough" is not enough.
        S = self.SLOTS
        copy_stream = torch.cuda.Stream(device=self.device)
        pin_img = [torch.empty((B,) + images.shape[1:],
                               dtype=images.dtype).pin_memory()
                   for _ in range(S)]
        pin_lbl = [torch.empty((B,), dtype=labels.dtype).pin_memory()
                   for _ in range(S)]
        events = [None] * S
        main = torch.cuda.current_stream(self.device)
        for bi, s0 in enumerate(range(0, idx.numel(), B)):
            k = bi % S
            if events[k] is not None:
                events[k].synchronize()   # prior H2D from this slot done
            sel = idx[s0:s0 + B]
            n = sel.numel()
            torch.index_select(images, 0, sel, out=pin_img[k][:n])
            torch.index_select(labels, 0, sel, out=pin_lbl[k][:n])
            with torch.cuda.stream(copy_stream):
                dev_i = pin_img[k][:n].to(self.device, non_blocking=True)
                dev_l = pin_lbl[k][:n].to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            events[k] = ev
            main.wait_stream(copy_stream)
            dev_i.record_stream(main)
            dev_l.record_stream(main)
            yield dev_i, dev_l


# ------------------------------------------------ device-resident datasets ---

_U64 = (1 << 64) - 1


def sample_params(seed: int, epoch: int, index, pad: int, hflip: bool):
    """Per-sample augmentation parameters ``(dx, dy, flip)`` as int64 numpy
    arrays — the counter hash of ``ops/hip/data.hip`` in numpy ``uint64``
    (arithmetic modulo 2^64).  Keyed by the DATASET index, so a sample's
    augmentation in an epoch is independent of batch size, rank and world
    size and is reproduced by a resumed run."""
    idx = np.atleast_1d(np.asarray(index)).astype(np.uint64)
    u = np.uint64
    s = np.full(1, int(seed) & _U64, dtype=np.uint64)
    e = np.full(1, int(epoch), dtype=np.uint64)
    key = (e << u(32)) | idx
    z = s + (key + u(1)) * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    span = u(2 * int(pad) + 1)
    dx = ((z & u(0xFFFF)) * span) >> u(16)
    dy = (((z >> u(16)) & u(0xFFFF)) * span) >> u(16)
    flip = ((z >> u(32)) & u(1)) if hflip else np.zeros_like(z)
    return dx.astype(np.int64), dy.astype(np.int64), flip.astype(np.int64)


def _mix_hash(seed: int, epoch: int, idx: np.ndarray) -> np.ndarray:
    u = np.uint64
    s = np.full(1, int(seed) & _U64, dtype=np.uint64)
    e = np.full(1, int(epoch), dtype=np.uint64)
    key = (e << u(32)) | idx
    z = s + (key + u(1)) * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    return z ^ (z >> u(31))


# seed offsets of the two CutMix hashes (ops/hip/data.hip, file header)
MIX_SEED_A = 0xD1B54A32D192ED03
MIX_SEED_B = 0x8CB92BA72F3D8DD7


def cutmix_threshold(prob: float) -> int:
    """Apply probability as the kernel's 16-bit threshold: a sample is mixed
    when its 16 hashed bits are below ``floor(prob * 65536 + 0.5)``."""
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"cutmix_prob must be in [0, 1], got {prob}")
    return int(math.floor(float(prob) * 65536.0 + 0.5))


CutMixParams = collections.namedtuple(
    "CutMixParams", "j apply box area lam raw")


def cutmix_params(seed: int, epoch: int, index, N: int, H: int, W: int,
                  prob: float) -> CutMixParams:
    """Per-sample CutMix parameters — the numpy mirror of ``mix_decode`` in
    ``ops/hip/data.hip`` (integers only, layout in that file's header).
    Keyed by (seed, epoch, DATASET index) like ``sample_params``.

    Returns int64 arrays: partner ``j`` in [0, N), ``apply`` (0/1), ``box``
    = (x0, y0, x1, y1) half-open and clipped to the image, ``area`` of the
    clipped box; ``lam`` float32 = (HW - area)/HW, 1 where not applied; and
    ``raw`` = (cx, cy, bw, bh), the centre and the unclipped box size.  The
    box and area are reported whether or not the sample is applied."""
    idx = np.atleast_1d(np.asarray(index)).astype(np.uint64)
    u = np.uint64
    z2 = _mix_hash(int(seed) + MIX_SEED_A, epoch, idx)
    z3 = _mix_hash(int(seed) + MIX_SEED_B, epoch, idx)
    j = ((z2 & u(0xFFFFFFFF)) * u(N)) >> u(32)
    v = (z2 >> u(32)).astype(np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)                 # exact floor sqrt
    r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    cx = (((z3 & u(0xFFFF)) * u(W)) >> u(16)).astype(np.int64)
    cy = ((((z3 >> u(16)) & u(0xFFFF)) * u(H)) >> u(16)).astype(np.int64)
    bits = ((z3 >> u(32)) & u(0xFFFF)).astype(np.int64)
    apply = (bits < cutmix_threshold(prob)).astype(np.int64)
    bw = (r * W) >> 16
    bh = (r * H) >> 16
    x0 = cx - bw // 2
    y0 = cy - bh // 2
    x1 = np.minimum(x0 + bw, W)
    y1 = np.minimum(y0 + bh, H)
    x0 = np.maximum(x0, 0)
    y0 = np.maximum(y0, 0)
    area = (x1 - x0) * (y1 - y0)
    hw = np.float32(H * W)
    lam = ((H * W - area * apply).astype(np.float32) / hw).astype(np.float32)
    return CutMixParams(j.astype(np.int64), apply, (x0, y0, x1, y1), area,
                        lam, (cx, cy, bw, bh))


class Augment:
    """Augmentation / normalisation config of ``DeviceBatchLoader``.

    ``crop_pad`` = P: random crop of the original size out of the image
    zero-padded by P pixels (torchvision ``RandomCrop(padding=P)``);
    ``hflip``: random horizontal flip; ``mean``/``std``: per-channel
    normalisation.  The kernel does no arithmetic on pixels — everything
    value-related is folded into the ``[C, 256]`` bf16 table of ``lut()``.
    ``cutmix_prob`` > 0 pastes, with that probability per sample, a hashed
    box of a partner sample (``cutmix_params``) and makes the loader yield
    ``MixedTarget`` labels."""

    def __init__(self, crop_pad: int = 0, hflip: bool = False,
                 mean=None, std=None, cutmix_prob: float = 0.0):
        if crop_pad < 0:
            raise ValueError("crop_pad must be >= 0")
        self.cutmix_prob = float(cutmix_prob)
        cutmix_threshold(self.cutmix_prob)       # range check
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together")
        self.crop_pad = int(crop_pad)
        self.hflip = bool(hflip)
        self.mean = None if mean is None else tuple(float(m) for m in mean)
        self.std = None if std is None else tuple(float(s) for s in std)

    def lut(self, channels: int) -> torch.Tensor:
        """[C, 256] bf16 table: value of raw byte u in channel c.  Without
        mean/std it is (u/255).to(bf16) — bit-for-bit the host path's cast
        of a k/255 image."""
        u = torch.arange(256, dtype=torch.float32) / 255.0
        t = u.unsqueeze(0).repeat(channels, 1)
        if self.mean is not None:
            if len(self.mean) != channels or len(self.std) != channels:
                raise ValueError(
                    f"mean/std need {channels} entries, got "
                    f"{len(self.mean)}/{len(self.std)}")
            mean = torch.tensor(self.mean, dtype=torch.float32).unsqueeze(1)
            std = torch.tensor(self.std, dtype=torch.float32).unsqueeze(1)
            t = (t - mean) / std
        return t.to(torch.bfloat16).contiguous()

    def __repr__(self):
        mix = f", cutmix_prob={self.cutmix_prob}" if self.cutmix_prob else ""
        return (f"Augment(crop_pad={self.crop_pad}, hflip={self.hflip}, "
                f"mean={self.mean}, std={self.std}{mix})")


def quantize_store(images: torch.Tensor, chunk: int = 1024) -> torch.Tensor:
    """[N,C,H,W] float in [0,1] -> [N,H,W,C] uint8 via round(x*255).  Exact
    for k/255 images (real MNIST/CIFAR files); anything else — the synthetic
    stand-ins — is quantised to 8 bits."""
    N, C, H, W = images.shape
    store = torch.empty((N, H, W, C), dtype=torch.uint8)
    for s0 in range(0, N, chunk):
        q = (images[s0:s0 + chunk].float() * 255.0).round_().clamp_(0, 255)
        store[s0:s0 + chunk] = q.to(torch.uint8).permute(0, 2, 3, 1)
    return store


def reference_batch(store: torch.Tensor, lut: torch.Tensor,
                    index: torch.Tensor, pad: int, hflip: bool, seed: int,
                    epoch: int) -> torch.Tensor:
    """CPU reference of the ``batch_gather_aug`` kernel: fp32 NCHW batch of
    ``lut.float()`` values.  Torchvision order (pad, crop, flip): output
    pixel (y, x) of a sample reads source (y + dy - P, xs + dx - P) with
    xs = W-1-x when flipped; outside the image the value is lut[c][0]."""
    N, H, W, C = store.shape
    index = index.clamp(0, N - 1)          # the kernel clamps too
    dx, dy, flip = sample_params(seed, epoch, index.numpy(), pad, hflip)
    dx, dy, flip = (torch.from_numpy(a) for a in (dx, dy, flip))
    ys = torch.arange(H).unsqueeze(0) + (dy - pad).unsqueeze(1)      # [B,H]
    xo = torch.arange(W).unsqueeze(0)
    xo = torch.where(flip.bool().unsqueeze(1), W - 1 - xo, xo)
    xs = xo + (dx - pad).unsqueeze(1)                                # [B,W]
    inside = (((ys >= 0) & (ys < H)).unsqueeze(2)
              & ((xs >= 0) & (xs < W)).unsqueeze(1))                 # [B,H,W]
    u = store[index.view(-1, 1, 1),
              ys.clamp(0, H - 1).unsqueeze(2),
              xs.clamp(0, W - 1).unsqueeze(1)]                       # [B,H,W,C]
    u = torch.where(inside.unsqueeze(3), u, torch.zeros_like(u)).long()
    out = lut.float()[torch.arange(C).view(1, 1, 1, C), u]
    return out.permute(0, 3, 1, 2).contiguous()


def reference_batch_cutmix(store: torch.Tensor, lut: torch.Tensor,
                           labels: torch.Tensor, index: torch.Tensor,
                           pad: int, hflip: bool, seed: int, epoch: int,
                           prob: float):
    """CPU reference of the ``batch_gather_cutmix`` kernel: ``(images,
    labels_a, labels_b, lam)`` with images = where(box, aug(j), aug(i)) —
    two ``reference_batch`` calls and a mask; the partner j carries its own
    (dx, dy, flip) of the epoch."""
    N, H, W, C = store.shape
    index = index.clamp(0, N - 1)
    mp = cutmix_params(seed, epoch, index.numpy(), N, H, W, prob)
    apply = torch.from_numpy(mp.apply).bool()
    partner = torch.where(apply, torch.from_numpy(mp.j), index)
    own = reference_batch(store, lut, index, pad, hflip, seed, epoch)
    other = reference_batch(store, lut, partner, pad, hflip, seed, epoch)
    x0, y0, x1, y1 = (torch.from_numpy(a).view(-1, 1, 1) for a in mp.box)
    ys = torch.arange(H).view(1, H, 1)
    xs = torch.arange(W).view(1, 1, W)
    mask = (apply.view(-1, 1, 1) & (xs >= x0) & (xs < x1)
            & (ys >= y0) & (ys < y1))                                # [B,H,W]
    images = torch.where(mask.unsqueeze(1), other, own)
    return (images, torch.index_select(labels, 0, index),
            torch.index_select(labels, 0, partner), torch.from_numpy(mp.lam))


class DeviceBatchLoader:
    """Batch loader over a device-resident uint8 copy of an in-memory
    dataset; same iteration contract as ``FastBatchLoader`` ((images,
    labels) batches in sampler order, last partial batch kept).

    On a GPU the dataset is quantised once (``round(x*255)``, HWC) and
    uploaded with its labels; per epoch the sampler's index list goes up as
    one int64 tensor; per batch ONE launch of ``ext.batch_gather_aug`` on
    the current stream gathers, crops, flips, normalises and writes the
    bf16 channels_last batch the stem conv consumes, plus the labels.  No
    host gather, no H2D copy, no cast/layout pass, no side stream.

    Without a GPU (``device`` None or a CPU device) the same batches come
    from ``reference_batch`` as fp32 NCHW — the tests' oracle and the CPU
    training path.

    With ``augment.cutmix_prob`` > 0 the batches are ``(images,
    MixedTarget)`` from ``ext.batch_gather_cutmix`` (CPU:
    ``reference_batch_cutmix``), still one launch per batch; with it off
    nothing changes, the same call as before builds the batch.

    The device path sees every dataset at 8 bits: real MNIST/CIFAR files
    (k/255 values) round-trip exactly, the synthetic stand-ins are
    quantised.  If the store would take more than half of the free device
    memory the loader prints one line and iterates a ``FastBatchLoader``
    instead (which cannot augment or normalise)."""

    def __init__(self, dataset, batch_size: int, sampler=None, device=None,
                 augment: Optional[Augment] = None, seed: int = 0):
        self.dataset = dataset
        self.batch_size = batch_size
        self.sampler = sampler
        self.device = device
        self.augment = augment if augment is not None else Augment()
        self.seed = int(seed)
        self.gpu = (device is not None and device.type == "cuda"
                    and torch.cuda.is_available())
        images = dataset.images
        N, C, H, W = images.shape
        self.lut = self.augment.lut(C)
        self._fallback = None
        self._ext = None
        if self.gpu:
            from ..ops import load_extension
            self._ext = load_extension(required=True)
            if self._ext is None:      # DDPX_FORCE_TORCH: no kernel, no loader
                raise RuntimeError("DeviceBatchLoader needs the _hip_ops "
                                   "extension on a GPU device")
            nbytes = N * C * H * W
            free, _ = torch.cuda.mem_get_info(device)
            if nbytes > free // 2:
                if self.augment.cutmix_prob > 0:
                    raise RuntimeError(
                        "CutMix needs the device-resident store, which does "
                        "not fit in half of the free device memory")
                print(f"[data] uint8 store of {nbytes / 2**20:.0f} MiB "
                      f"exceeds half of the free device memory "
                      f"({free / 2**20:.0f} MiB free); using the host "
                      f"FastBatchLoader path (no augmentation/normalisation)")
                self._fallback = FastBatchLoader(
                    dataset, batch_size, sampler=sampler, pin_memory=True,
                    device=device)
                return
        store = quantize_store(images)
        labels = dataset.labels.to(torch.int64).contiguous()
        if self.gpu:
            self.store = store.to(device)
            self.labels = labels.to(device)
            self.lut = self.lut.to(device)
        else:
            self.store = store
            self.labels = labels

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        if self._fallback is not None:
            yield from self._fallback
            return
        if self.sampler is not None:
            idx = torch.as_tensor(list(self.sampler), dtype=torch.long)
        else:
            idx = torch.arange(len(self.dataset), dtype=torch.long)
        epoch = int(getattr(self.sampler, "epoch", 0) or 0)
        aug = self.augment
        B = self.batch_size
        if aug.cutmix_prob > 0:
            yield from self._iter_cutmix(idx, epoch)
            return
        if not self.gpu:
            for s0 in range(0, idx.numel(), B):
                sel = idx[s0:s0 + B]
                yield (reference_batch(self.store, self.lut, sel,
                                       aug.crop_pad, aug.hflip, self.seed,
                                       epoch),
                       torch.index_select(self.labels, 0, sel))
            return
        idx_dev = idx.to(self.device)     # one upload per epoch
        seed = self.seed & _U64           # the binding takes it as int64 bits
        seed = seed - (1 << 64) if seed >> 63 else seed
        for s0 in range(0, idx.numel(), B):
            images, labels = self._ext.batch_gather_aug(
                self.store, self.labels, idx_dev[s0:s0 + B], self.lut,
                aug.crop_pad, aug.hflip, seed, epoch)
            yield images, labels

    def _iter_cutmix(self, idx, epoch):
        from ..ops.functional import MixedTarget
        aug = self.augment
        B = self.batch_size
        if not self.gpu:
            for s0 in range(0, idx.numel(), B):
                images, la, lb, lam = reference_batch_cutmix(
                    self.store, self.lut, self.labels, idx[s0:s0 + B],
                    aug.crop_pad, aug.hflip, self.seed, epoch,
                    aug.cutmix_prob)
                yield images, MixedTarget(la, lb, lam)
            return
        idx_dev = idx.to(self.device)     # one upload per epoch
        seed = self.seed & _U64           # the binding takes it as int64 bits
        seed = seed - (1 << 64) if seed >> 63 else seed
        thresh = cutmix_threshold(aug.cutmix_prob)
        for s0 in range(0, idx.numel(), B):
            images, la, lb, lam = self._ext.batch_gather_cutmix(
                self.store, self.labels, idx_dev[s0:s0 + B], self.lut,
                aug.crop_pad, aug.hflip, seed, epoch, thresh)
            yield images, MixedTarget(la, lb, lam)
