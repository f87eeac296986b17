"""run.py — CLI + process-group init entry point.

API-compatible with the reference entry point (reference run.py:7-32):
identical 10 flags and defaults, ``--local_rank`` injected by the launcher
(``python -m ddp_tricks_amd.launch`` or torchrun-style LOCAL_RANK env),
then process-group init over RCCL (backend "nccl" IS RCCL on ROCm) and
``train(args)``.  Falls back to gloo on CPU-only machines and fills in
single-process rendezvous defaults so ``python run.py`` works standalone.
"""
import argparse
import os

import torch
import torch.distributed as dist

from ddp_tricks_amd.utils.train import train


def parse_args():
    parser = argparse.ArgumentParser()
    parser.add_argument("-n", "--exp_name", default="DDP_warmup", type=str,
                        help="name of experiment")
    parser.add_argument("-l", "--learning_rate", default=1e-1, type=float,
                        help="learning rate")
    parser.add_argument("-b", "--batch_size", default=1024, type=int,
                        help="batch size")
    parser.add_argument("-e", "--epochs", default=500, type=int,
                        help="epochs")
    parser.add_argument("-w", "--warmup_epochs", default=10, type=int,
                        help="epochs for warmup")
    parser.add_argument("-t", "--warmup_type", default="linear", type=str,
                        help="warmup type")
    parser.add_argument("-s", "--seed_num", default=42, type=int,
                        help="number of random seed")
    parser.add_argument("-d", "--data_path", default="./datasets/", type=str,
                        help="path of dataset")
    parser.add_argument("-p", "--model_path", default="./experiment_model/",
                        type=str, help="path of model")
    parser.add_argument("--local_rank", type=int, default=None,
                        help="local rank for DistributedDataParallel")
    # extensions beyond the reference's 10-flag contract
    parser.add_argument("--model", default="toy_net", type=str,
                        help="model registry name (toy_net, vgg16, resnet18, "
                             "resnet34, resnet50)")
    parser.add_argument("--dataset", default="mnist", type=str,
                        help="dataset registry name (mnist, cifar10, "
                             "imagenet_synthetic)")
    parser.add_argument("--resume", action="store_true",
                        help="save/load the sidecar resume checkpoint")
    parser.add_argument("--clip_grad_norm", default=0.0, type=float,
                        help="clip the global gradient 2-norm to this value "
                             "(0 = off)")
    parser.add_argument("--device_data", action="store_true",
                        help="keep the dataset on the GPU as uint8 and build "
                             "each batch with one fused HIP kernel")
    parser.add_argument("--augment", default="none", type=str,
                        choices=("none", "flip", "crop_flip"),
                        help="train-set augmentation (crop_flip: random crop "
                             "with 4-pixel padding + horizontal flip); "
                             "implies --device_data on GPU")
    parser.add_argument("--normalize", action="store_true",
                        help="normalise train and valid images with the "
                             "dataset's per-channel MEAN/STD")
    parser.add_argument("--sync_bn", action="store_true",
                        help="convert every BatchNorm to SyncBatchNorm: "
                             "batch statistics over all ranks, one small "
                             "gather per layer and direction")
    parser.add_argument("--label_smoothing", default=0.0, type=float,
                        help="label smoothing of the training loss, in "
                             "[0, 1); validation loss stays unsmoothed")
    parser.add_argument("--cutmix_prob", default=0.0, type=float,
                        help="per-sample CutMix probability on the train "
                             "loader (alpha = 1 boxes); implies "
                             "--device_data on GPU")
    parser.add_argument("--optimizer", default="sgd", type=str,
                        choices=("sgd", "lars", "adamw", "lamb"),
                        help="sgd: fused nesterov SGD; lars: the same step "
                             "with layer-wise trust ratios on the weights "
                             "(BN parameters and biases are not adapted); "
                             "adamw: fused AdamW; lamb: Adam's direction "
                             "with layer-wise trust ratios (pass an "
                             "Adam-scale -l with these two)")
    parser.add_argument("--weight_decay", default=0.0, type=float,
                        help="L2 weight decay (with --optimizer lars: on the "
                             "adapted tensors only; with adamw / lamb: "
                             "decoupled, not on BN parameters and biases)")
    parser.add_argument("--adam_beta1", default=0.9, type=float,
                        help="adamw / lamb: first-moment decay")
    parser.add_argument("--adam_beta2", default=0.999, type=float,
                        help="adamw / lamb: second-moment decay")
    parser.add_argument("--adam_eps", default=1e-8, type=float,
                        help="adamw / lamb: epsilon of the denominator")
    parser.add_argument("--lars_eta", default=0.001, type=float,
                        help="LARS trust coefficient")
    parser.add_argument("--dropout", default=0.0, type=float,
                        help="dropout probability of the model's dropout "
                             "slots (vgg16's classifier); masks are a "
                             "counter hash of (seed, rank, epoch, call), "
                             "fused into the linear epilogue (0 = off)")
    args = parser.parse_args()
    if args.local_rank is None:
        args.local_rank = int(os.environ.get("LOCAL_RANK", 0))
    return args


def main():
    args = parse_args()
    print(f"Running DDP on rank: {args.local_rank}")

    # single-process fallback rendezvous (container hostnames may not resolve
    # — always rendezvous on loopback)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    os.environ.setdefault("RANK", str(args.local_rank))
    os.environ.setdefault("WORLD_SIZE", "1")

    if torch.cuda.is_available():
        torch.cuda.set_device(args.local_rank)
        backend = "nccl"  # RCCL on ROCm
    else:
        backend = "gloo"
    dist.init_process_group(backend=backend, init_method="env://")
    try:
        train(args)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
