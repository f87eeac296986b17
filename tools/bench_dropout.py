"""Fused Linear+ReLU+dropout against the composition it replaces
(docs/KERNELS.md, "Fused dropout").

Per junction shape [M,K] -> N, forward + backward (dx, dw, db) of

  fused        ops.linear_relu_dropout: linear_act_fwd, relu_drop_bwd,
               linear_dgrad / linear_wgrad / col_sum
  composed     ops.linear + torch.relu + nn.Dropout: the same HIP linear
               kernels with ATen's relu, bernoulli mask, multiplies and
               threshold_backward around them

The composed rows run in a process of their own with
DDPX_ALLOW_TORCH_FALLBACK=1 (the only way to run that path today); the
parent prints both.  Also the standalone kernels at 2^21 elements against
``torch.nn.functional.dropout``.

Method: bf16 activations, fp32 master weight (its bf16 operand is cached,
as in a training step), p = 0.5.  WARMUP calls, then device events around
STEPS back-to-back fwd+bwd calls, median of REPEATS; launch gaps and the
Python side are included, as in a training step.
"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, STEPS, REPEATS = 5, 20, 5
SHAPES = [(256, 25088, 4096), (256, 4096, 4096), (256, 512, 512)]
NUMEL = 1 << 21
P = 0.5


def _time(fn):
    """median, min, max us per call over REPEATS x STEPS back-to-back"""
    import torch
    reps = []
    for _ in range(REPEATS):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) * 1e3 / STEPS)
    reps.sort()
    return reps[len(reps) // 2], reps[0], reps[-1]


def _row(name, t):
    print(f"  {name:22s} median {t[0]:9.1f} us (min {t[1]:.1f} max {t[2]:.1f}; "
          f"{REPEATS} x {STEPS} back-to-back calls)", flush=True)


def _junctions(mode):
    import torch

    from ddp_tricks_amd import ops
    from ddp_tricks_amd.ops.modules import Linear
    dev = torch.device("cuda:0")
    ops.load_extension(required=True)
    ops.dropout_rng.seed(0, rank=0)
    for M, K, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        lin = Linear(K, N).to(dev)
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16) \
            .requires_grad_()
        dy = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
        if mode == "fused":
            drop = ops.Dropout(P).train()

            def fwd():
                return ops.linear_relu_dropout(lin, drop, x)
        else:
            drop = torch.nn.Dropout(P).train()

            def fwd():
                return drop(torch.relu(lin(x)))

        def step():
            x.grad = lin.weight.grad = lin.bias.grad = None
            fwd().backward(dy)

        print(f"[{M},{K}] -> {N}, fwd + bwd:", flush=True)
        _row(mode, _time(step))
        assert bool(torch.isfinite(lin.weight.grad).all())
        del lin, x, dy
        torch.cuda.empty_cache()


def _standalone():
    import torch

    from ddp_tricks_amd import ops
    from ddp_tricks_amd.ops.functional import dropout_scale, dropout_threshold
    ext = ops.load_extension(required=True)
    dev = torch.device("cuda:0")
    thr = dropout_threshold(P)
    scale = dropout_scale(thr)
    print(f"standalone kernels, {NUMEL} elements:", flush=True)
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = torch.randn(NUMEL, device=dev).to(dtype)
        _row(f"dropout_fwd {tag}",
             _time(lambda: ext.dropout_fwd(x, thr, scale, 12345)))
        _row(f"dropout_bwd {tag}",
             _time(lambda: ext.dropout_bwd(x, thr, scale, 12345)))
        _row(f"relu_dropout_fwd {tag}",
             _time(lambda: ext.relu_dropout_fwd(x, thr, scale, 12345)))
        _row(f"F.dropout fwd {tag}",
             _time(lambda: torch.nn.functional.dropout(x, P, True)))
    x = torch.randn(NUMEL, device=dev).to(torch.bfloat16)
    y = torch.relu(torch.randn(NUMEL, device=dev)).to(torch.bfloat16)
    _row("relu_drop_bwd bf16", _time(lambda: ext.relu_drop_bwd(x, y, scale)))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--composed":
        _junctions("composed")
        return
    _junctions("fused")
    _standalone()
    env = dict(os.environ, DDPX_ALLOW_TORCH_FALLBACK="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__),
                        "--composed"], env=env, cwd=REPO)
    if r.returncode != 0:
        raise SystemExit(f"composed child failed with {r.returncode}")


if __name__ == "__main__":
    main()
