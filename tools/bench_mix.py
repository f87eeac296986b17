"""Measurements of label smoothing / CutMix (docs/KERNELS.md, "Label
smoothing and CutMix").  Two sub-commands, each one GPU process:

  kernel   per-launch time of the batch kernel with CutMix off
           (ext.batch_gather_aug, the unchanged launch) and on
           (ext.batch_gather_cutmix, prob 0.5 and 1.0) at the three real
           batch shapes, crop_flip + normalise; same method as
           bench_device_data.py kernel: 20 warm-up launches, then device
           events around 200 back-to-back launches, median of 5 repeats
  ce       ce_fwd / ce_bwd against ce_mix_fwd / ce_mix_bwd (smoothing 0.1,
           random target pairs) at bf16 [1024,10] and [256,1000], same method
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, LAUNCHES, REPEATS = 20, 200, 5


def _time(fn):
    """median, min, max us per call over REPEATS x LAUNCHES back-to-back"""
    import torch
    reps = []
    for _ in range(REPEATS):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    reps.sort()
    return reps[len(reps) // 2], reps[0], reps[-1]


def bench_kernel():
    import torch

    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.utils.data import (CIFAR10, MNIST, Augment,
                                           SyntheticImageNet,
                                           cutmix_threshold)
    shapes = [
        ("mnist_b1024", 60000, 28, 28, 1, 1024, MNIST),
        ("cifar_b256", 50000, 32, 32, 3, 256, CIFAR10),
        ("imagenet_b256", 1024, 224, 224, 3, 256, SyntheticImageNet),
    ]
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    for name, N, H, W, C, B, ds in shapes:
        g = torch.Generator().manual_seed(0)
        store = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8,
                              generator=g).to(dev)
        labels = torch.randint(0, 10, (N,), generator=g).to(dev)
        lut = Augment(mean=ds.MEAN, std=ds.STD).lut(C).to(dev)
        idx = torch.randperm(N, generator=g)[:B].to(dev)
        variants = [("off", lambda: ext.batch_gather_aug(
            store, labels, idx, lut, 4, True, 42, 1))]
        for prob in (0.5, 1.0):
            th = cutmix_threshold(prob)
            variants.append((f"cutmix_{prob}", lambda th=th:
                             ext.batch_gather_cutmix(store, labels, idx, lut,
                                                     4, True, 42, 1, th)))
        for vname, fn in variants:
            us, lo, hi = _time(fn)
            print(f"{name:14s} {vname:11s} median {us:8.2f} us/launch "
                  f"(min {lo:.2f} max {hi:.2f}; {REPEATS} x {LAUNCHES} "
                  f"back-to-back launches, launch gaps included)", flush=True)
        del store


def bench_ce():
    import torch

    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for B, C in ((1024, 10), (256, 1000)):
        x = torch.randn(B, C, generator=g).to(torch.bfloat16).to(dev)
        a = torch.randint(0, C, (B,), generator=g).to(dev)
        b = torch.randint(0, C, (B,), generator=g).to(dev)
        lam = torch.rand(B, generator=g).to(dev)
        dloss = torch.ones((), device=dev)
        _, lse = ext.ce_fwd(x, a)
        rows = [
            ("ce_fwd", lambda: ext.ce_fwd(x, a)),
            ("ce_mix_fwd", lambda: ext.ce_mix_fwd(x, a, b, lam, 0.1)),
            ("ce_bwd", lambda: ext.ce_bwd(x, a, lse, dloss)),
            ("ce_mix_bwd", lambda: ext.ce_mix_bwd(x, a, b, lam, lse, dloss,
                                                  0.1)),
        ]
        for name, fn in rows:
            us, lo, hi = _time(fn)
            print(f"[{B},{C}] bf16 {name:11s} median {us:7.2f} us/call "
                  f"(min {lo:.2f} max {hi:.2f}; {REPEATS} x {LAUNCHES} "
                  f"back-to-back calls, launch gaps and output allocation "
                  f"included; fwd = row kernel + mean kernel)", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernel":
        bench_kernel()
    elif what == "ce":
        bench_ce()
    else:
        sys.exit(__doc__)
