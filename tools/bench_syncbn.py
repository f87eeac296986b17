"""Cost of the SyncBatchNorm split path against the plain fused BN kernels.

Usage (on a GPU box):  python tools/bench_syncbn.py [--reps 100] [--rounds 3]

For every BN shape of ResNet-50 (B = 32 and 256) and Toy_Net (B = 1024)
it times, with HIP events after a warm-up and alternating the two variants
inside each round so drift hits both:

  plain fwd   bn_fwd_train                 (partial, combine, apply)
  sync  fwd   bn_sync_local + bn_sync_fwd  (partial, pack, finalize, apply)
  plain bwd   bn_bwd                       (partial, combine, dx)
  sync  bwd   bn_sync_bwd_local + bn_sync_bwd_dx
                                           (partial, pack, coef, dx)

at world size 1 with the gather replaced by a view of the local row, so
the figure is the added kernel launches only — the collective itself and
any cross-device latency are NOT in it.  Prints the median over rounds
and the min..max spread; the last column is the added microseconds per BN
per direction.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ddp_tricks_amd.ops import load_extension  # noqa: E402

CL = torch.channels_last
BF = torch.bfloat16

SHAPES = [(f"r50 B={B} {hw}x{hw}x{C}", B, C, hw)
          for B in (32, 256)
          for hw, C in ((56, 256), (28, 512), (14, 1024), (7, 2048))]
SHAPES += [(f"toy B=1024 {hw}x{hw}x{C}", 1024, C, hw)
           for hw, C in ((26, 64), (24, 128), (10, 256), (8, 512))]


def time_op(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1000.0  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_syncbn needs a GPU"
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    print(f"{'shape':24s} {'dir':3s} {'plain us':>20s} {'sync us':>20s} "
          f"{'added us':>9s}")
    for name, B, C, hw in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, C, hw, hw, device=dev, generator=g).to(BF) \
            .contiguous(memory_format=CL)
        dy = torch.randn(B, C, hw, hw, device=dev, generator=g).to(BF) \
            .contiguous(memory_format=CL)
        gamma = torch.ones(C, device=dev)
        beta = torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def plain_fwd():
            return ext.bn_fwd_train(x, gamma, beta, rm, rv, 0.1, 1e-5, True)

        def sync_fwd():
            row = ext.bn_sync_local(x)
            return ext.bn_sync_fwd(x, row.view(1, -1), gamma, beta, rm, rv,
                                   0.1, 1e-5, True)
        _, sm, si, mask = plain_fwd()
        o = sync_fwd()
        assert torch.equal(o[1], sm) and torch.equal(o[2], si)
        count = o[4]

        def plain_bwd():
            return ext.bn_bwd(x, dy, gamma, sm, si, mask, True, False)

        def sync_bwd():
            row = ext.bn_sync_bwd_local(x, dy, sm, si, mask, True)
            return ext.bn_sync_bwd_dx(x, dy, gamma, sm, si, mask, True,
                                      row.view(1, -1), count, False)
        assert torch.equal(sync_bwd()[0], plain_bwd()[0])
        for tag, plain, sync in (("fwd", plain_fwd, sync_fwd),
                                 ("bwd", plain_bwd, sync_bwd)):
            tp, ts = [], []
            for _ in range(args.rounds):
                tp.append(time_op(plain, args.reps))
                ts.append(time_op(sync, args.reps))
            mp, ms = statistics.median(tp), statistics.median(ts)
            print(f"{name:24s} {tag:3s} "
                  f"{mp:8.1f} ({min(tp):.1f}..{max(tp):.1f}) "
                  f"{ms:8.1f} ({min(ts):.1f}..{max(ts):.1f}) "
                  f"{ms - mp:+9.1f}", flush=True)
        del x, dy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
