"""train(args) — full training orchestration.

Re-implements the reference trainer's exact wiring (reference
utils/train.py:23-118) on the MI355X-native stack: our MNIST pipeline +
DistributedSampler, our Toy_Net (HIP kernels on GPU), FusedSGD + Lookahead,
our amp runtime, our RCCL-bucketed DDP, our tfevents writer, identical
epoch loop / scheduler gating / early stopping / best-checkpoint rule.

Behavioral quirks preserved: epoch 0 trains at LR 0;
warmup steps while ``epoch <= warmup_epochs``; cosine branch freezes after
warmup; plateau patience 6 / factor 0.1 on valid loss; EarlyStopping
patience 30; unsharded validation on every rank; train metrics rank-local;
rank-0 best-valid-acc gated ``torch.save(module.state_dict())`` to
``{model_path}/{exp_name}.pt`` (37-key fp32 layout).
"""
from __future__ import annotations

import math
import os
import time

import torch
from torch.utils.data import DataLoader

from .. import amp
from ..models import build_model, model_accepts
from ..ops import dropout_rng
from ..ops.optim import (FusedAdamW, FusedLAMB, FusedLARS, FusedSGD,
                         decay_param_groups, lars_param_groups)
from ..parallel.ddp import DistributedDataParallel as DDP
from .callbacks import EarlyStopping, same_seeds
from .data import (DATASETS, Augment, CudaPrefetcher, DeviceBatchLoader,
                   DistributedSampler, FastBatchLoader)
from .engine import iterate_loader
from .lookahead import Lookahead
from .schedulers import ReduceLROnPlateau, WarmupLambdaLR
from .tboard import SummaryWriter


# --augment choices -> (crop_pad, hflip); crop_flip is the standard CIFAR
# recipe (random crop with 4-pixel padding + horizontal flip)
AUGMENT_MODES = {"none": (0, False), "flip": (0, True), "crop_flip": (4, True)}


def _resolve_device(local_rank):
    if torch.cuda.is_available():
        rank = local_rank if local_rank is not None and local_rank >= 0 else 0
        torch.cuda.set_device(rank)
        return torch.device("cuda", rank)
    return torch.device("cpu")


def resolve_model_kwargs(args, model_name: str, dataset_name: str) -> dict:
    """Constructor keywords of ``--model`` for this run: the caller's
    ``args.model_kwargs``, the CIFAR head/stem defaults, and ``--dropout``
    (only when > 0, so the default builds exactly the default model)."""
    model_kwargs = dict(getattr(args, "model_kwargs", None) or {})
    if model_name.startswith("resnet") and dataset_name == "cifar10":
        model_kwargs.setdefault("num_classes", 10)
        model_kwargs.setdefault("cifar_stem", True)
    if model_name.startswith("vgg") and dataset_name == "cifar10":
        model_kwargs.setdefault("num_classes", 10)
        model_kwargs.setdefault("cifar_head", True)
    dropout = float(getattr(args, "dropout", 0.0) or 0.0)
    if dropout < 0.0:
        raise ValueError("--dropout must be >= 0")
    if dropout > 0:
        if not model_accepts(model_name, "dropout"):
            raise ValueError(f"--dropout: model {model_name!r} has no "
                             "dropout layers (its constructor takes no "
                             "'dropout' argument)")
        model_kwargs["dropout"] = dropout
    return model_kwargs


def train(args):
    local_rank = getattr(args, "local_rank", 0) or 0
    device = _resolve_device(local_rank)

    # Extensions over the reference's 10-flag contract:
    # --model / --dataset select from the registries; --resume restarts
    # from the sidecar checkpoint.  Defaults reproduce the reference.
    model_name = getattr(args, "model", None) or "toy_net"
    dataset_name = getattr(args, "dataset", None) or "mnist"
    model_kwargs = resolve_model_kwargs(args, model_name, dataset_name)
    # the dropout stream is keyed by (seed, rank); the process group (if
    # any) is up by now
    dropout_rng.seed(args.seed_num)
    Dataset = DATASETS[dataset_name]

    # Data pipeline (reference utils/train.py:24-30: sharded train loader,
    # UNSHARDED valid loader evaluated in full on every rank)
    train_set = Dataset(root=args.data_path, train=True, download=True)
    train_sampler = DistributedSampler(train_set)
    same_seeds(args.seed_num)
    pin = device.type == "cuda"
    dev_arg = device if pin else None
    # Opt-in device-resident data path (extension): --device_data keeps the
    # dataset on the GPU as uint8 and builds batches with one HIP kernel;
    # --augment / --normalize need that loader (the host path can express
    # neither), so they imply it — on CPU its reference implementation runs.
    augment_mode = getattr(args, "augment", None) or "none"
    if augment_mode not in AUGMENT_MODES:
        raise ValueError(f"unknown augment mode {augment_mode!r}")
    normalize = bool(getattr(args, "normalize", False))
    # --cutmix_prob (train loader only) lives in the same batch kernel, so
    # it implies the device loader the way --augment does
    cutmix_prob = float(getattr(args, "cutmix_prob", 0.0) or 0.0)
    if not 0.0 <= cutmix_prob <= 1.0:
        raise ValueError("--cutmix_prob must be in [0, 1]")
    device_data = (bool(getattr(args, "device_data", False))
                   or augment_mode != "none" or normalize or cutmix_prob > 0)
    if device_data and not hasattr(train_set, "images"):
        raise ValueError("--device_data/--augment/--normalize/--cutmix_prob "
                         "need an in-memory dataset (one with an .images "
                         "tensor)")
    if device_data:
        norm = dict(mean=Dataset.MEAN, std=Dataset.STD) if normalize else {}
        crop_pad, hflip = AUGMENT_MODES[augment_mode]
        mix = dict(cutmix_prob=cutmix_prob) if cutmix_prob > 0 else {}
        train_loader = DeviceBatchLoader(
            train_set, args.batch_size, sampler=train_sampler,
            device=dev_arg, seed=args.seed_num,
            augment=Augment(crop_pad=crop_pad, hflip=hflip, **norm, **mix))
    elif hasattr(train_set, "images"):   # in-memory tensors: vectorized path
        train_loader = FastBatchLoader(train_set, args.batch_size,
                                       sampler=train_sampler, pin_memory=pin,
                                       device=dev_arg)
    else:
        train_loader = DataLoader(train_set, batch_size=args.batch_size,
                                  shuffle=False, pin_memory=pin,
                                  sampler=train_sampler)
    valid_set = Dataset(root=args.data_path, train=False, download=True)
    if getattr(train_set, "synthetic", False) \
            and not getattr(valid_set, "synthetic", True):
        # Coherence guard: the train images are absent (synthetic stand-in)
        # but real valid files exist — validating a synthetic-trained model
        # on real digits reports chance accuracy and would silently distort
        # EarlyStopping/plateau/best-checkpoint decisions.  Keep the pair
        # learnable: synthetic valid drawn from the same class templates.
        print("[data] train split is synthetic but real valid files exist; "
              "using the synthetic valid split for a coherent train/valid "
              "pair")
        valid_set = Dataset(root=args.data_path, train=False, download=False,
                            synthetic=True)
    if device_data:    # the valid loader never augments
        valid_loader = DeviceBatchLoader(valid_set, args.batch_size,
                                         device=dev_arg, seed=args.seed_num,
                                         augment=Augment(**norm))
    elif hasattr(valid_set, "images"):
        valid_loader = FastBatchLoader(valid_set, args.batch_size,
                                       pin_memory=pin, device=dev_arg)
    else:
        valid_loader = DataLoader(valid_set, batch_size=args.batch_size,
                                  shuffle=False, pin_memory=pin)
    if device.type == "cuda":
        # FastBatchLoader already yields device tensors with its own
        # one-ahead copy stream; only wrap generic DataLoaders
        own_h2d = (FastBatchLoader, DeviceBatchLoader)
        if not isinstance(train_loader, own_h2d):
            train_loader = CudaPrefetcher(train_loader, device)
        if not isinstance(valid_loader, own_h2d):
            valid_loader = CudaPrefetcher(valid_loader, device)

    print(f"Now Training: {args.exp_name}")

    # Model (seeded identically on all ranks before the DDP broadcast —
    # reference utils/train.py:34-36, README rationale)
    same_seeds(args.seed_num)
    model = build_model(model_name, **model_kwargs)
    model = model.to(device)
    if getattr(args, "sync_bn", False):
        # opt-in cross-rank BatchNorm statistics; parameters and buffers
        # stay the same objects, so everything below is unaffected
        from ..parallel.sync_bn import convert_sync_batchnorm
        model = convert_sync_batchnorm(model)

    os.makedirs(os.path.join(args.model_path, "logs"), exist_ok=True)
    latest_model_path = os.path.join(args.model_path, args.exp_name)
    # --optimizer / --weight_decay / --lars_eta / --adam_* (extension); the
    # defaults build the reference's SGD(lr, momentum=0.9, nesterov=True)
    optimizer_name = getattr(args, "optimizer", None) or "sgd"
    weight_decay = float(getattr(args, "weight_decay", 0.0) or 0.0)
    if weight_decay < 0.0:
        raise ValueError("--weight_decay must be >= 0")
    if optimizer_name == "sgd":
        optimizer = FusedSGD(model.parameters(), lr=args.learning_rate,
                             momentum=0.9, weight_decay=weight_decay,
                             nesterov=True)
    elif optimizer_name == "lars":
        # layer-wise trust ratios on the weights; BN scale/shift and biases
        # take the plain SGD step without decay
        lars_eta = float(getattr(args, "lars_eta", None) or 0.001)
        optimizer = FusedLARS(lars_param_groups(model, weight_decay),
                              lr=args.learning_rate, momentum=0.9,
                              nesterov=True, trust_coefficient=lars_eta)
    elif optimizer_name in ("adamw", "lamb"):
        # Adam-class steps: --weight_decay is decoupled and skips BN
        # scale/shift and biases (for lamb they also take the plain AdamW
        # step); -l must be an Adam-scale rate
        def flag(name, default):
            value = getattr(args, name, None)
            return default if value is None else float(value)
        betas = (flag("adam_beta1", 0.9), flag("adam_beta2", 0.999))
        adam_eps = flag("adam_eps", 1e-8)
        cls = FusedAdamW if optimizer_name == "adamw" else FusedLAMB
        optimizer = cls(decay_param_groups(model, weight_decay),
                        lr=args.learning_rate, betas=betas, eps=adam_eps,
                        weight_decay=weight_decay)
    else:
        raise ValueError(f"unknown optimizer {optimizer_name!r}")
    lookahead = Lookahead(optimizer=optimizer, k=10, alpha=0.5)
    from ..ops.functional import cross_entropy_loss as loss_function
    # --label_smoothing binds into the TRAINING loss only; validation keeps
    # the plain hard-target loss so valid_loss (plateau scheduler, early
    # stopping) stays comparable with runs that do not smooth
    label_smoothing = float(getattr(args, "label_smoothing", 0.0) or 0.0)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError("--label_smoothing must be in [0, 1)")
    train_loss_function = loss_function
    if label_smoothing > 0:
        import functools
        train_loss_function = functools.partial(
            loss_function, label_smoothing=label_smoothing)
    best_valid_acc = 0

    # LR warmup lambda (reference utils/train.py:48-51, incl. the dead
    # cosine decay quirk — the caller only steps warmup while
    # epoch <= warmup_epochs)
    if args.warmup_type == "linear":
        def warm_up(epoch):
            return epoch / args.warmup_epochs if epoch <= args.warmup_epochs else 1
    elif args.warmup_type == "cosine":
        def warm_up(epoch):
            if epoch <= args.warmup_epochs:
                return epoch / args.warmup_epochs
            return 0.5 * (math.cos((epoch - args.warmup_epochs)
                                   / (args.epochs - args.warmup_epochs) * math.pi) + 1)
    else:
        raise ValueError(f"unknown warmup_type {args.warmup_type!r}")
    scheduler_wu = WarmupLambdaLR(optimizer=optimizer, lr_lambda=warm_up)
    scheduler_re = ReduceLROnPlateau(optimizer=optimizer, mode="min",
                                     factor=0.1, patience=6, verbose=True)
    early_stopping = EarlyStopping(patience=30, verbose=True)

    # amp before DDP wrap (required order — SURVEY Appendix A.12)
    clip_grad_norm = float(getattr(args, "clip_grad_norm", 0.0) or 0.0)
    model, apex_optimizer = amp.initialize(model, optimizers=lookahead,
                                           opt_level="O1",
                                           max_grad_norm=clip_grad_norm)
    parallel_model = DDP(model)

    # Resume from the sidecar checkpoint (extension; the reference saves
    # best weights only and has no resume path — SURVEY §5.4).  Every rank
    # loads the same file, so state stays rank-consistent.
    start_epoch = 0
    resume_path = f"{latest_model_path}.resume.pt"
    resume_on = bool(getattr(args, "resume", False))
    if resume_on and os.path.exists(resume_path):
        ck = torch.load(resume_path, map_location=device, weights_only=False)
        parallel_model.module.load_state_dict(ck["model"])
        apex_optimizer.load_state_dict(ck["optimizer"])
        scheduler_wu.load_state_dict(ck["scheduler_wu"])
        scheduler_re.load_state_dict(ck["scheduler_re"])
        early_stopping.load_state_dict(ck["early_stopping"])
        amp.load_state_dict(ck.get("amp", {}))
        best_valid_acc = ck["best_valid_acc"]
        start_epoch = ck["epoch"] + 1
        from ..ops.functional import clear_weight_cache
        clear_weight_cache()
        print(f"resumed {args.exp_name} at epoch {start_epoch}")

    if local_rank == 0:
        tb = SummaryWriter(os.path.join(args.model_path, "logs", args.exp_name))

    for epoch in range(start_epoch, args.epochs):
        epoch_start_time = time.time()
        train_sampler.set_epoch(epoch)
        dropout_rng.set_epoch(epoch)   # restarts the per-epoch call counter

        parallel_model.train()
        train_loss, train_acc, curr_lr = iterate_loader(
            loader=train_loader, model=parallel_model,
            loss_function=train_loss_function, local_rank=local_rank,
            apex_optimizer=apex_optimizer, training=True)

        parallel_model.eval()
        with torch.no_grad():
            valid_loss, valid_acc = iterate_loader(
                loader=valid_loader, model=parallel_model,
                loss_function=loss_function, local_rank=local_rank,
                apex_optimizer=None, training=False)

        if local_rank == 0:
            tb.add_scalar("LR", curr_lr, epoch)
            tb.add_scalars("Loss", {"train": train_loss, "valid": valid_loss}, epoch)
            tb.add_scalars("Acc", {"train": train_acc, "valid": valid_acc}, epoch)

        clip_info = ""
        if clip_grad_norm > 0:
            gstats = iterate_loader.grad_norm_stats
            if local_rank == 0:
                tb.add_scalar("GradNorm", gstats["mean"], epoch)
                tb.add_scalar("GradClipFrac", gstats["clipped_frac"], epoch)
            clip_info = (f", grad_norm: {gstats['mean']:.4f}, "
                         f"clipped: {100.0 * gstats['clipped_frac']:.1f}%")

        phase_info = ""
        # DDPX_PHASE_TIMERS=1; the engine caches PhaseTimers
        # per device (events/streams are device-bound)
        tcache = getattr(iterate_loader, "_timers", None) or {}
        tm = tcache.get(device)
        if tm is not None:
            phase_info = f", phases[{tm.format()}]"
            tm.reset()
        print(f"epoch: {epoch:03d}/{args.epochs}, "
              f"time: {time.time() - epoch_start_time:.2f}s, "
              f"learning_rate: {curr_lr}, "
              f"train_loss: {train_loss:.4f}, train_acc: {train_acc:.4f}, "
              f"valid_loss: {valid_loss:.4f}, valid_acc: {valid_acc:.4f}"
              f"{phase_info}{clip_info}")

        # scheduler gating exactly as the reference (utils/train.py:104-106)
        if epoch <= args.warmup_epochs:
            scheduler_wu.step()
        scheduler_re.step(valid_loss)
        early_stopping(valid_loss)
        if early_stopping.early_stop:
            break

        if local_rank == 0 and valid_acc > best_valid_acc:
            best_valid_acc = valid_acc
            torch.save(parallel_model.module.state_dict(),
                       f"{latest_model_path}.pt")

        if local_rank == 0 and resume_on:
            torch.save({
                "epoch": epoch,
                "model": parallel_model.module.state_dict(),
                "optimizer": apex_optimizer.state_dict(),
                "scheduler_wu": scheduler_wu.state_dict(),
                "scheduler_re": scheduler_re.state_dict(),
                "early_stopping": early_stopping.state_dict(),
                "amp": amp.state_dict(),
                "best_valid_acc": best_valid_acc,
            }, resume_path)

    if local_rank == 0:
        tb.close()
