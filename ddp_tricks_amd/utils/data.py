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
"""
from __future__ import annotations

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
