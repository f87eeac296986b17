"""Measurements of the device-resident data path (docs/KERNELS.md,
"Device-resident datasets").  Three sub-commands, each one GPU process tree:

  kernel          per-launch time of ext.batch_gather_aug at the three real
                  batch shapes (device events around 200 back-to-back launches)
  loader          train-epoch wall time at ms resolution: the trainer's stack
                  and iterate_loader, fed alternately by FastBatchLoader and
                  DeviceBatchLoader in ONE process
  epochs toy|r18  run.py epoch wall time as printed, host path vs
                  --device_data vs --device_data --augment crop_flip
                  --normalize, alternating fresh processes (synthetic data)
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["DDPX_OFFLINE"] = "1"
os.environ["DDPX_NO_TQDM"] = "1"


# ----------------------------------------------------------------- kernel ---

def bench_kernel():
    import torch

    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.utils.data import (CIFAR10, MNIST, Augment,
                                           SyntheticImageNet)
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
        for vname, pad, flip, norm in (("plain", 0, False, False),
                                       ("crop_flip_norm", 4, True, True)):
            aug = Augment(mean=ds.MEAN, std=ds.STD) if norm else Augment()
            lut = aug.lut(C).to(dev)
            reps = []
            for rep in range(5):
                idx = torch.randperm(N, generator=g)[:B].to(dev)
                for _ in range(20):
                    ext.batch_gather_aug(store, labels, idx, lut, pad, flip,
                                         42, rep)
                torch.cuda.synchronize()
                n = 200
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    ext.batch_gather_aug(store, labels, idx, lut, pad, flip,
                                         42, rep)
                e1.record()
                torch.cuda.synchronize()
                reps.append(e0.elapsed_time(e1) * 1e3 / n)
            reps.sort()
            us = reps[len(reps) // 2]
            byts = B * H * W * C * 3     # 1 B read + 2 B written per element
            print(f"{name:14s} {vname:15s} median {us:8.2f} us/launch "
                  f"(min {reps[0]:.2f} max {reps[-1]:.2f}; 5 x 200 "
                  f"back-to-back launches, launch gaps included)  "
                  f"{byts / us / 1e3:8.1f} GB/s of {byts / 1e6:.2f} MB moved",
                  flush=True)
        del store


# ----------------------------------------------------------------- loader ---

def bench_loader():
    import torch
    import torch.distributed as dist

    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.ops.functional import (clear_weight_cache,
                                               cross_entropy_loss)
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    from ddp_tricks_amd.utils.data import (DATASETS, Augment,
                                           DeviceBatchLoader,
                                           DistributedSampler,
                                           FastBatchLoader)
    from ddp_tricks_amd.utils.engine import iterate_loader
    from ddp_tricks_amd.utils.lookahead import Lookahead

    configs = [
        ("toy_net", {}, "mnist", 1024, 7),
        ("resnet18", {"num_classes": 10, "cifar_stem": True}, "cifar10",
         256, 4),
    ]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1)
    summary = []
    for model_name, kw, ds_name, B, rounds in configs:
        amp._state.__init__()
        clear_weight_cache()
        DS = DATASETS[ds_name]
        train_set = DS(root="/nonexistent", train=True, synthetic=True)
        sampler = DistributedSampler(train_set)
        same_seeds(42)
        model = build_model(model_name, **kw).to(dev)
        opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9,
                       nesterov=True)
        la = Lookahead(optimizer=opt, k=10, alpha=0.5)
        model, aopt = amp.initialize(model, optimizers=la, opt_level="O1")
        pm = DDP(model)
        loaders = {
            "host": FastBatchLoader(train_set, B, sampler=sampler,
                                    pin_memory=True, device=dev),
            "device": DeviceBatchLoader(train_set, B, sampler=sampler,
                                        device=dev, augment=Augment(),
                                        seed=42),
            "device_aug": DeviceBatchLoader(
                train_set, B, sampler=sampler, device=dev, seed=42,
                augment=Augment(crop_pad=4, hflip=True, mean=DS.MEAN,
                                std=DS.STD)),
        }
        times = {k: [] for k in loaders}
        pm.train()
        epoch = 0
        for r in range(rounds + 1):          # round 0 = warm-up, dropped
            for name, loader in loaders.items():
                sampler.set_epoch(epoch)
                epoch += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss, _, _ = iterate_loader(
                    loader=loader, model=pm, loss_function=cross_entropy_loss,
                    local_rank=0, apex_optimizer=aopt, training=True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r:
                    times[name].append(dt)
                print(f"{model_name} round {r} {name}: {dt * 1e3:.1f} ms "
                      f"loss {loss:.4f}", flush=True)
        n = len(train_set)
        steps = len(loaders["host"])
        summary.append(f"## {model_name}/{ds_name} B={B}: train epoch of {n} "
                       f"images, {steps} steps, {rounds} alternating rounds "
                       f"after 1 warm-up round")
        for name, t in times.items():
            med = statistics.median(t)
            summary.append(
                f"{name:11s} median {med * 1e3:8.1f} ms  min "
                f"{min(t) * 1e3:8.1f}  max {max(t) * 1e3:8.1f}  "
                f"({med / steps * 1e3:.3f} ms/step, "
                f"{n / med / 1e3:.1f}k img/s)")
        del loaders, train_set
    dist.destroy_process_group()
    print("\n".join(summary))


# ----------------------------------------------------------------- epochs ---

EPOCH_CONFIGS = {
    "toy": (["--model", "toy_net", "--dataset", "mnist", "-b", "1024",
             "-e", "7", "-w", "2"], 3),
    "r18": (["--model", "resnet18", "--dataset", "cifar10", "-b", "256",
             "-e", "6", "-w", "2"], 2),
}
EPOCH_VARIANTS = [
    ("host", []),
    ("device", ["--device_data"]),
    ("device_aug", ["--device_data", "--augment", "crop_flip", "--normalize"]),
]


def bench_epochs(name):
    base, rounds = EPOCH_CONFIGS[name]
    env = dict(os.environ)
    times = {v: [] for v, _ in EPOCH_VARIANTS}
    port = 29510
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for v, flags in EPOCH_VARIANTS:
                port += 1
                env["MASTER_PORT"] = str(port)
                args = ["-n", f"{name}_{v}_{r}"] + base + flags
                cmd = [sys.executable, os.path.join(REPO, "run.py"),
                       "-p", tmp, "-d", os.path.join(tmp, "no_data")] + args
                p = subprocess.run(cmd, env=env, capture_output=True,
                                   text=True, timeout=280, cwd=REPO)
                print(f"### round {r} variant {v}: run.py {' '.join(args)} "
                      f"(rc {p.returncode})")
                print("\n".join(l for l in p.stdout.splitlines()
                                if l.startswith("epoch:")), flush=True)
                if p.returncode != 0:   # stop: nothing more runs on the GPU
                    print(p.stderr[-4000:])
                    return 1
                times[v].append([float(x) for x in re.findall(
                    r"epoch: \d+/\d+, time: ([\d.]+)s", p.stdout)])
    print(f"## {name}: per-epoch wall time [s] as printed by run.py "
          f"(train + valid), epoch 0 skipped")
    for v, _ in EPOCH_VARIANTS:
        flat = [t for ep in times[v] for t in ep[1:]]
        print(f"{v:11s} n={len(flat)} median={statistics.median(flat):.3f} "
              f"min={min(flat):.3f} max={max(flat):.3f} per-run medians="
              f"{[round(statistics.median(ep[1:]), 3) for ep in times[v]]}")
    return 0


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernel":
        bench_kernel()
    elif what == "loader":
        bench_loader()
    elif what == "epochs" and len(sys.argv) > 2 and sys.argv[2] in EPOCH_CONFIGS:
        sys.exit(bench_epochs(sys.argv[2]))
    else:
        sys.exit(__doc__)
