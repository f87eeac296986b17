"""Step time of FusedLARS against FusedSGD (docs/KERNELS.md, "Fused LARS").

One GPU process.  For Toy_Net, ResNet-50 and VGG-16 the parameters are
synthetic fp32 tensors with the model's shape list (the model is built on
the meta device for its shapes only; no forward is run), gradients are
random, momentum 0.9 + nesterov, weight decay 5e-4.  Per model:

  sgd          FusedSGD over all tensors (one group)
  lars         FusedLARS(lars_param_groups): tensors with ndim > 1 adapted,
               the 1-D ones through the plain SGD launch
  lars_all     FusedLARS with every tensor adapted (the kernels' own cost)

Method: 20 warm-up steps, then device events around 100 back-to-back
optimizer.step() calls, median of 5 repeats; launch gaps and the Python
side of the step are included, as in a training step.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, STEPS, REPEATS = 20, 100, 5
MT_MAX = 32          # tensors per launch group (ops/hip/elementwise.hip)


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


def _groups(n):
    return (n + MT_MAX - 1) // MT_MAX


def main():
    import torch

    from ddp_tricks_amd.ops import (FusedLARS, FusedSGD, lars_param_groups,
                                    load_extension)
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    ch = ext.MT_CHUNK
    for name in ("toy_net", "resnet50", "vgg16"):
        shapes = _shapes(name)
        g = torch.Generator(device=dev).manual_seed(0)

        def make():
            ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g))
                  for s in shapes]
            for p in ps:
                p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
            return ps

        n_ad = sum(len(s) > 1 for s in shapes)
        n_pl = len(shapes) - n_ad
        numel = sum(torch.Size(s).numel() for s in shapes)
        chunks = sum((torch.Size(s).numel() + ch - 1) // ch for s in shapes)
        small = sum(torch.Size(s).numel() <= ch for s in shapes)
        print(f"{name}: {len(shapes)} tensors ({n_ad} with ndim > 1), "
              f"{numel * 4 / 2 ** 20:.1f} MiB fp32, {chunks} chunks, "
              f"{small} tensors of one chunk or less", flush=True)
        kw = dict(lr=1e-3, momentum=0.9, nesterov=True)
        rows = []
        ps = make()
        rows.append(("sgd", FusedSGD(ps, weight_decay=5e-4, **kw),
                     _groups(len(ps))))
        ps = make()
        holder = torch.nn.ParameterList(ps)
        rows.append(("lars", FusedLARS(lars_param_groups(holder, 5e-4), **kw),
                     3 * _groups(n_ad) + _groups(n_pl)))
        ps = make()
        rows.append(("lars_all", FusedLARS(ps, weight_decay=5e-4, **kw),
                     3 * _groups(len(ps))))
        base = None
        for rname, opt, launches in rows:
            us, lo, hi = _time(opt.step)
            base = base or us
            print(f"  {rname:9s} median {us:8.1f} us/step (min {lo:.1f} max "
                  f"{hi:.1f}; {launches:2d} launches/step; {us / base:.2f}x "
                  f"sgd; {REPEATS} x {STEPS} back-to-back steps)", flush=True)
            finite = all(bool(torch.isfinite(p).all())
                         for grp in opt.param_groups for p in grp["params"])
            assert finite, f"{name} {rname}: non-finite parameters"
        del rows, ps, holder
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
