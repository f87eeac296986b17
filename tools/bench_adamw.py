"""Step time of FusedAdamW and FusedLAMB against torch.optim.AdamW
(docs/KERNELS.md, "Fused AdamW and LAMB").

For Toy_Net, ResNet-50 and VGG-16 the parameters are synthetic fp32 tensors
with the model's shape list (the model is built on the meta device for its
shapes only; no forward is run), gradients are random, betas (0.9, 0.999),
eps 1e-8, weight decay 0.05.  Per model:

  fused_adamw    FusedAdamW over all tensors (one group)
  fused_lamb     FusedLAMB with every tensor adapted (the kernels' own cost)
  torch_fused    torch.optim.AdamW(fused=True)
  torch_foreach  torch.optim.AdamW(foreach=True)

Every row runs in a fresh child process under its own time limit, one
after the other; the first row that fails or runs out of time ends the
run.  Method: 10 warm-up steps, then device events around 50 back-to-back
optimizer.step() calls, median of 5 repeats; launch gaps and the Python
side of the step are included, as in a training step.  Bytes per element
and step: AdamW reads g, p, m, v and writes p, m, v (28 B); LAMB's moments
pass reads four and writes two arrays, its step pass reads three and
writes one (40 B).
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, STEPS, REPEATS = 10, 50, 5
ROW_TIMEOUT = 120    # seconds per child
MODELS = ("toy_net", "resnet50", "vgg16")
ROWS = ("fused_adamw", "fused_lamb", "torch_fused", "torch_foreach")
BYTES = {"fused_adamw": 28, "fused_lamb": 40, "torch_fused": 28,
         "torch_foreach": 28}


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


def _shapes(name):
    import torch

    from ddp_tricks_amd.models import build_model
    with torch.device("meta"):
        model = build_model(name)
    return [tuple(p.shape) for p in model.parameters()]


def child(model, row):
    import torch

    from ddp_tricks_amd.ops import FusedAdamW, FusedLAMB, load_extension
    load_extension(required=True)
    dev = torch.device("cuda:0")
    shapes = _shapes(model)
    g = torch.Generator(device=dev).manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g))
          for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    if row == "fused_adamw":
        opt = FusedAdamW(ps, **kw)
    elif row == "fused_lamb":
        opt = FusedLAMB(ps, **kw)
    elif row == "torch_fused":
        opt = torch.optim.AdamW(ps, fused=True, **kw)
    else:
        opt = torch.optim.AdamW(ps, foreach=True, **kw)
    us, lo, hi = _time(opt.step)
    assert all(bool(torch.isfinite(p).all()) for p in ps), "non-finite"
    numel = sum(p.numel() for p in ps)
    print(json.dumps(dict(model=model, row=row, tensors=len(ps), numel=numel,
                          us=us, lo=lo, hi=hi)), flush=True)


def main():
    base = {}
    for model in MODELS:
        for row in ROWS:
            try:
                r = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), "--child",
                     model, row], cwd=REPO, capture_output=True, text=True,
                    timeout=ROW_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"{model} {row}: no result in {ROW_TIMEOUT} s; "
                      "stopping", flush=True)
                return 1
            if r.returncode != 0:
                print(f"{model} {row}: exit {r.returncode}; stopping\n"
                      f"{r.stderr[-2000:]}", flush=True)
                return 1
            d = json.loads(r.stdout.strip().splitlines()[-1])
            if row == ROWS[0]:
                print(f"{model}: {d['tensors']} tensors, "
                      f"{d['numel'] * 4 / 2 ** 20:.1f} MiB fp32", flush=True)
                base[model] = d["us"]
            tbs = d["numel"] * BYTES[row] / (d["us"] * 1e-6) / 1e12
            print(f"  {row:13s} median {d['us']:8.1f} us/step (min "
                  f"{d['lo']:.1f} max {d['hi']:.1f}; {tbs:5.2f} TB/s at "
                  f"{BYTES[row]} B/element; {d['us'] / base[model]:.2f}x "
                  f"fused_adamw; {REPEATS} x {STEPS} back-to-back steps)",
                  flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
