"""Micro-benchmark of the HIP conv kernels at the workload's shapes.

Usage (on a GPU box):  python tools/bench_kernels.py [--resnet]
                       python tools/bench_kernels.py --bn | --bnpool
                       python tools/bench_kernels.py --clip
                       python tools/bench_kernels.py --wgradbias
                       python tools/bench_kernels.py --wgraddma [--leaves wt3]
                       python tools/bench_kernels.py --dgradtaps
                       python tools/bench_kernels.py --kwalk

Times conv fwd/dgrad/wgrad per shape with HIP events (200 reps after 20
warmup) and prints achieved TFLOP/s next to microseconds, so kernel A/B
decisions are measurements, not guesses.  DDPX_WGRAD_V forces a conv wgrad
leaf for comparison: wt / wt3 (wide_dma at the automatic depth / 32-deep),
wp / wq (wide_pair 64- / 32-deep), s or sb / s6 (sb_pair 32- / 64-deep).
The extension rejects every other value, so --leaves takes only these
spellings; a child given anything else stops at its first wgrad call.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ddp_tricks_amd.ops import load_extension  # noqa: E402

CL = torch.channels_last

TOYNET = [
    # (name, N, C, H, W, K, R, stride, pad)
    ("conv2", 1024, 64, 26, 26, 128, 3, 1, 0),
    ("conv3", 1024, 128, 12, 12, 256, 3, 1, 0),
    ("conv4", 1024, 256, 10, 10, 512, 3, 1, 0),
    ("conv1", 1024, 1, 28, 28, 64, 3, 1, 0),
    ("conv1p8", 1024, 8, 28, 28, 64, 3, 1, 0),
]
RESNET = [
    ("r18s1", 256, 64, 32, 32, 64, 3, 1, 1),
    ("r18s2", 256, 64, 32, 32, 128, 3, 2, 1),
    ("r18d2", 256, 64, 32, 32, 128, 1, 2, 0),
    ("r50c1", 256, 64, 56, 56, 64, 1, 1, 0),
    ("r50c3", 256, 64, 56, 56, 256, 1, 1, 0),
    ("r50l3", 256, 256, 14, 14, 1024, 1, 1, 0),
    ("stem50", 64, 8, 224, 224, 64, 7, 2, 3),
]


def time_op(fn, reps=200, warmup=20):
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


def bench_functional(shapes, reps):
    """Times the autograd-level conv path (true dispatch: 1x1 GEMM route,
    pad8 stems, fused wgrad variants) — fwd and full bwd per shape."""
    import torch.nn as nn

    from ddp_tricks_amd.ops import functional as F_ops
    dev = torch.device("cuda:0")
    print(f"{'shape':8s} {'op':6s} {'us':>9s} {'TFLOP/s':>9s}")
    for name, N, C, H, W, K, R, stride, pad in shapes:
        P = (H + 2 * pad - R) // stride + 1
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16)\
            .contiguous(memory_format=CL).requires_grad_(True)
        w = nn.Parameter(torch.randn(K, C, R, R, device=dev))
        dy = torch.randn(N, K, P, P, device=dev).to(torch.bfloat16)\
            .contiguous(memory_format=CL)
        flops = 2.0 * N * P * P * K * C * R * R

        us = time_op(lambda: F_ops.conv2d(x.detach(), w, None, stride, pad),
                     reps)
        print(f"{name:8s} {'Ffwd':6s} {us:9.1f} {flops/us/1e6:9.1f}")

        def fb():
            y = F_ops.conv2d(x, w, None, stride, pad)
            y.backward(dy)
        us = time_op(fb, reps // 2)
        print(f"{name:8s} {'Ffb':6s} {us:9.1f} {3*flops/us/1e6:9.1f}")


BN_SHAPES = [
    ("stem", 256, 64, 112, 112),
    ("l1", 256, 256, 56, 56),
    ("l1b", 256, 64, 56, 56),
    ("l2", 256, 512, 28, 28),
    ("l3", 256, 1024, 14, 14),
    ("l4", 256, 2048, 7, 7),
    ("toy2", 1024, 128, 24, 24),
]


def bench_bn(reps):
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    print(f"{'shape':6s} {'op':10s} {'us':>9s} {'GB/s':>8s}")
    for name, N, C, H, W in BN_SHAPES:
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn_like(x).contiguous(memory_format=CL)
        g = torch.rand(C, device=dev) + 0.5
        b = torch.randn(C, device=dev)
        rm = torch.zeros(C, device=dev)
        rv = torch.ones(C, device=dev)
        nbytes = x.numel() * 2
        us = time_op(lambda: ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5,
                                              True, None), reps)
        # fwd: read x twice (partial+apply) + write y + mask
        print(f"{name:6s} {'fwd_train':10s} {us:9.1f} {(3.06*nbytes)/us/1e3:8.0f}")
        y, sm, si, mask = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True, None)
        us = time_op(lambda: ext.bn_bwd(x, dy, g, sm, si, mask, True, False),
                     reps)
        # bwd: partial reads x,dy,mask; dx reads x,dy,mask writes dx
        print(f"{name:6s} {'bwd':10s} {us:9.1f} {(5.13*nbytes)/us/1e3:8.0f}")


BNPOOL_SHAPES = [
    # Toy_Net's two BN(fuse_relu) -> MaxPool2d(2) junctions at B=1024
    ("toy2", 1024, 128, 24, 24),
    ("toy4", 1024, 512, 8, 8),
]


def bench_bnpool(reps):
    """BN+ReLU -> 2x2 max-pool junction, fwd and bwd: the unfused kernel
    pair against the fused bn_*_pool2 entry points (statistics pass
    included on both sides)."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    print(f"{'shape':6s} {'op':6s} {'unfused us':>11s} {'fused us':>9s}")
    for name, N, C, H, W in BNPOOL_SHAPES:
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
        dyp = torch.randn(N, C, H // 2, W // 2, device=dev).to(torch.bfloat16)\
            .contiguous(memory_format=CL)
        g = torch.rand(C, device=dev) + 0.5
        b = torch.randn(C, device=dev)
        rm = torch.zeros(C, device=dev)
        rv = torch.ones(C, device=dev)

        def fwd_unfused():
            y = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True, None)[0]
            return ext.maxpool2x2_fwd(y)
        us_u = time_op(fwd_unfused, reps)
        us_f = time_op(lambda: ext.bn_fwd_train_pool2(x, g, b, rm, rv, 0.1,
                                                      1e-5), reps)
        print(f"{name:6s} {'fwd':6s} {us_u:11.1f} {us_f:9.1f}")

        y, sm, si, mask = ext.bn_fwd_train(x, g, b, rm, rv, 0.1, 1e-5, True, None)
        _, idx = ext.maxpool2x2_fwd(y)
        _, sm2, si2, code = ext.bn_fwd_train_pool2(x, g, b, rm, rv, 0.1, 1e-5)

        def bwd_unfused():
            dy = ext.maxpool2x2_bwd(dyp, idx, H, W)
            return ext.bn_bwd(x, dy, g, sm, si, mask, True, False)
        us_u = time_op(bwd_unfused, reps)
        us_f = time_op(lambda: ext.bn_bwd_pool2(x, dyp, g, sm2, si2, code),
                       reps)
        print(f"{name:6s} {'bwd':6s} {us_u:11.1f} {us_f:9.1f}")


def _time_alternating(variants, rounds=30, inner=10, warmup=5):
    """Per-call microseconds of each variant, measured alternately in one
    process: every round times `inner` back-to-back calls of each variant
    with device events.  Returns {name: (median, min, max)} over rounds."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            samples[name].append(s.elapsed_time(e) / inner * 1000.0)
    out = {}
    for k, v in samples.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def bench_clip(rounds):
    """Gradient-norm clipping: what the fused path adds to the unscale and
    SGD passes, against the standalone square-sum/finalize/scale passes, at
    the real gradient payloads (default 4 MiB DDP bucket flats)."""
    from ddp_tricks_amd.models import build_model
    from ddp_tricks_amd.parallel.ddp import DistributedDataParallel as DDP
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    ch = ext.MT_CHUNK
    print(f"{'payload':10s} {'MB':>7s} {'variant':26s} {'med us':>9s} "
          f"{'min':>9s} {'max':>9s}")
    for name in ("toy_net", "resnet50", "vgg16"):
        model = build_model(name).to(dev)
        ddp = DDP(model)
        flats = ddp.bucket_flats()
        params = [p for p in model.parameters() if p.requires_grad]
        for p in params:
            if p.grad is None:      # grads are views into the bucket flats
                raise RuntimeError("DDP did not attach bucket-view grads")
        for f in flats:
            f.normal_()
        grads = [p.grad for p in params]
        bufs = [torch.zeros_like(p) for p in params]
        n = sum((f.numel() + ch - 1) // ch for f in flats)
        partials = torch.zeros(n, device=dev)
        out = torch.zeros(2, device=dev)
        stats = torch.zeros(4, device=dev)
        fi = torch.zeros(1, device=dev)
        one = torch.ones(1, device=dev)
        mb = sum(f.numel() for f in flats) * 4 / 1e6
        # inv_scale 1, lr 0, coefficient 1: values stay put over the reps

        def unscale_plain():
            ext.multi_tensor_unscale(flats, fi, 1.0)

        def unscale_norm():
            ext.multi_tensor_unscale(flats, fi, 1.0, partials)
            ext.norm_finalize(partials, n, 1.0, fi, out, stats)

        def sgd_plain():
            ext.fused_sgd(params, grads, bufs, 0.0, 0.9, 0.0, 1.0, fi)

        def sgd_scaled():
            ext.fused_sgd(params, grads, bufs, 0.0, 0.9, 0.0, 1.0, fi, one)

        def standalone():
            ext.multi_tensor_sqsum(flats, partials)
            ext.norm_finalize(partials, n, 1.0, fi, out, stats)
            ext.multi_tensor_scale(flats, one, fi)

        res = _time_alternating({
            "a0 unscale": unscale_plain,
            "a1 unscale+sqsum+finalize": unscale_norm,
            "b0 sgd": sgd_plain,
            "b1 sgd+device scale": sgd_scaled,
            "c  sqsum+finalize+scale": standalone,
        }, rounds=rounds)
        for k, (med, lo, hi) in res.items():
            print(f"{name:10s} {mb:7.1f} {k:26s} {med:9.1f} {lo:9.1f} "
                  f"{hi:9.1f}")
        fused = (res["a1 unscale+sqsum+finalize"][0] - res["a0 unscale"][0]
                 + res["b1 sgd+device scale"][0] - res["b0 sgd"][0])
        print(f"{name:10s} {mb:7.1f} fused adds {fused:.1f} us; standalone "
              f"costs {res['c  sqsum+finalize+scale'][0]:.1f} us")
        del model, ddp, flats, params, grads, bufs
        torch.cuda.empty_cache()


def bench_wgradbias(rounds):
    """Weight + bias gradient of the four Toy_Net convs: conv2d_wgrad
    followed by col_sum (two passes over dy) against conv2d_wgrad_bias (db
    out of the wgrad and combine launches), and the wgrad alone."""
    from ddp_tricks_amd.ops.functional import _nhwc_2d
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    print(f"{'shape':8s} {'dy MB':>7s} {'variant':22s} {'med us':>9s} "
          f"{'min':>9s} {'max':>9s} {'dy TB/s':>8s}")
    for name, N, C, H, W, K, R, stride, pad in TOYNET:
        if name == "conv1p8":
            continue
        P = (H + 2 * pad - R) // stride + 1
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=CL)
        dy = torch.randn(N, K, P, P, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=CL)
        dy2 = _nhwc_2d(dy)
        mb = dy.numel() * 2 / 1e6

        def wgrad_only():
            ext.conv2d_wgrad(dy, x, R, R, stride, pad)

        def unfused():
            ext.conv2d_wgrad(dy, x, R, R, stride, pad)
            ext.col_sum(dy2)

        def fused():
            ext.conv2d_wgrad_bias(dy, x, R, R, stride, pad)

        res = _time_alternating({
            "wgrad": wgrad_only,
            "wgrad + col_sum": unfused,
            "wgrad_bias": fused,
        }, rounds=rounds)
        for k, (med, lo, hi) in res.items():
            print(f"{name:8s} {mb:7.1f} {k:22s} {med:9.1f} {lo:9.1f} "
                  f"{hi:9.1f} {mb / med:8.2f}")


def _wgraddma_child():
    """One leaf's side of --wgraddma: DDPX_WGRAD_V is read once per
    process, so each leaf lives in a process of its own.  Protocol on
    stdin/stdout, one line each way: ``setup <shape index>`` allocates the
    operands and warms up, ``run <0|1> <inner>`` answers the per-call
    microseconds of `inner` back-to-back calls (1 = with bias), ``quit``."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    x = dy = geo = None
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "setup":
            name, N, C, H, W, K, R, stride, pad = TOYNET[int(cmd[1])]
            P = (H + 2 * pad - R) // stride + 1
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(N, C, H, W, device=dev, generator=g) \
                .to(torch.bfloat16).contiguous(memory_format=CL)
            dy = torch.randn(N, K, P, P, device=dev, generator=g) \
                .to(torch.bfloat16).contiguous(memory_format=CL)
            geo = (R, R, stride, pad)
            for _ in range(5):
                ext.conv2d_wgrad(dy, x, *geo)
                ext.conv2d_wgrad_bias(dy, x, *geo)
            torch.cuda.synchronize()
            print("ok", flush=True)
            continue
        fn = ext.conv2d_wgrad_bias if cmd[1] == "1" else ext.conv2d_wgrad
        inner = int(cmd[2])
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn(dy, x, *geo)
        e.record()
        e.synchronize()
        print(f"{s.elapsed_time(e) / inner * 1000.0:.3f}", flush=True)


def bench_wgraddma(rounds, extra, inner=10):
    """wgrad of the four Toy_Net convs, with and without bias: the
    wide_pair leaf of the shape's depth class (wp / wq) against the LDS-DMA
    staged leaf (wt), plus any further DDPX_WGRAD_V letters in `extra`.
    Every leaf runs in a fresh child process; rounds alternate between the
    children, device events around `inner` calls, median/min/max over
    `rounds`.  This process never opens the GPU.  conv1 (C = 1) takes the
    stem kernel under every letter: it is the control row."""
    import subprocess
    leaves = ["wp", "wq", "wt"] + [v for v in extra if v]
    kids = {}
    for leaf in leaves:
        env = dict(os.environ)
        env["DDPX_WGRAD_V"] = leaf
        kids[leaf] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--wgraddma-child"],
            env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
            text=True, bufsize=1)

    def ask(leaf, msg):
        kids[leaf].stdin.write(msg + "\n")
        kids[leaf].stdin.flush()
        ans = kids[leaf].stdout.readline().strip()
        if not ans:
            raise RuntimeError(f"child {leaf} died on '{msg}'")
        return ans

    try:
        print(f"{'shape':8s} {'bias':>4s} {'leaf':6s} {'med us':>9s} "
              f"{'min':>9s} {'max':>9s} {'TFLOP/s':>8s}")
        for idx, (name, N, C, H, W, K, R, stride, pad) in enumerate(TOYNET):
            if name == "conv1p8":
                continue
            P = (H + 2 * pad - R) // stride + 1
            flops = 2.0 * N * P * P * K * C * R * R
            old = "wp" if R * R * C >= 1152 else "wq"
            use = [v for v in leaves if v not in ("wp", "wq") or v == old]
            for leaf in use:
                ask(leaf, f"setup {idx}")
            for bias in (0, 1):
                samples = {v: [] for v in use}
                for _ in range(rounds):
                    for leaf in use:
                        samples[leaf].append(
                            float(ask(leaf, f"run {bias} {inner}")))
                for leaf in use:
                    v = sorted(samples[leaf])
                    med = v[len(v) // 2]
                    print(f"{name:8s} {bias:4d} {leaf:6s} {med:9.1f} "
                          f"{v[0]:9.1f} {v[-1]:9.1f} {flops / med / 1e6:8.1f}",
                          flush=True)
    finally:
        for p in kids.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.close()
            except OSError:
                pass
        for p in kids.values():
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()


def bench_dgradtaps(rounds, groups):
    """Stride-1 dgrad of Toy_Net's conv2, conv3 and conv4 at B = 1024: the
    raster row order (group 0) against the tap-uniform order at each G in
    `groups`, alternated in one process (`group` is an argument, not an
    environment variable).  Device events around 10 calls, median/min/max
    over `rounds`; next to it the plan's K-tile count relative to raster,
    which is what the time would be if every K-tile cost the same."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    print(f"{'shape':8s} {'group':>5s} {'plan':8s} {'med us':>9s} {'min':>9s} "
          f"{'max':>9s} {'vs raster':>9s} {'model':>7s}")
    for name, N, C, H, W, K, R, stride, pad in TOYNET[:3]:
        P = (H + 2 * pad - R) // stride + 1
        g = torch.Generator(device=dev).manual_seed(0)
        dy = torch.randn(N, K, P, P, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        wt2 = torch.randn(C, R * R * K, device=dev, generator=g) \
            .to(torch.bfloat16)
        geo = (N, C, H, W, R, R, stride, pad)
        variants, plans = {}, {}
        for G in groups:
            variants[G] = (lambda G=G: ext.conv2d_dgrad(dy, wt2, *geo,
                                                        None, G))
            plans[G] = ext.conv2d_dgrad_plan(N, C, H, W, K, R, R, stride,
                                             pad, G)
        ref = ext.conv2d_dgrad(dy, wt2, *geo, None, 0)
        for G in groups:
            if not torch.equal(variants[G](), ref):
                raise RuntimeError(f"{name} group {G}: dx differs from raster")
        res = _time_alternating(variants, rounds=rounds)
        for G in groups:
            med, lo, hi = res[G]
            pname, _, issued, raster = plans[G]
            print(f"{name:8s} {G:5d} {pname:8s} {med:9.1f} {lo:9.1f} "
                  f"{hi:9.1f} {med / res[groups[0]][0]:9.3f} "
                  f"{issued / raster:7.3f}", flush=True)
        del dy, wt2, ref, variants
        torch.cuda.empty_cache()


def bench_kwalk(rounds):
    """K loop of k_conv_gemm: per-chunk address decode (kwalk 0) against the
    scalar tap walk (kwalk 1), alternated in one process (`kwalk` is an
    argument).  Forward goes through conv2d_fwd_stats as the training step
    calls it; dgrad runs the row order the automatic plan picks at B = 1024
    (conv2 raster, conv3 and conv4 tap-uniform at G = 128).  Controls: a 3x3
    pad-1 stride-1 and a 3x3 pad-1 stride-2 ResNet layer.  Outputs are
    checked equal before timing; 30 warm-up calls, then device events
    around 10 calls, median/min/max over `rounds`."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    by_name = {s[0]: s for s in TOYNET + RESNET}
    rows = [("fwd", n, 0) for n in ("conv2", "conv3", "conv4")]
    rows += [("dgrad", "conv2", 0), ("dgrad", "conv3", 128),
             ("dgrad", "conv4", 128)]
    rows += [("fwd", "r18s1", 0), ("dgrad", "r18s1", 0), ("fwd", "r18s2", 0)]
    print(f"{'op':6s} {'shape':8s} {'kwalk':>5s} {'plan':7s} {'med us':>9s} "
          f"{'min':>9s} {'max':>9s} {'vs decode':>9s} {'TFLOP/s':>8s}")
    for op, name, G in rows:
        _, N, C, H, W, K, R, stride, pad = by_name[name]
        P = (H + 2 * pad - R) // stride + 1
        flops = 2.0 * N * P * P * K * C * R * R
        g = torch.Generator(device=dev).manual_seed(0)
        if op == "fwd":
            x = torch.randn(N, C, H, W, device=dev, generator=g) \
                .to(torch.bfloat16).contiguous(memory_format=CL)
            w = torch.randn(K, C, R, R, device=dev, generator=g) \
                .to(torch.bfloat16).contiguous(memory_format=CL)
            call = (lambda kw: ext.conv2d_fwd_stats(x, w, None, stride, pad,
                                                    kw))
            plan = (lambda kw: ext.conv2d_kloop_plan(0, N, C, H, W, K, R, R,
                                                     stride, pad, kw))
        else:
            dy = torch.randn(N, K, P, P, device=dev, generator=g) \
                .to(torch.bfloat16).contiguous(memory_format=CL)
            wt2 = torch.randn(C, R * R * K, device=dev, generator=g) \
                .to(torch.bfloat16)
            call = (lambda kw: [ext.conv2d_dgrad(dy, wt2, N, C, H, W, R, R,
                                                 stride, pad, None, G, kw)])
            plan = (lambda kw: ext.conv2d_kloop_plan(1, N, C, H, W, K, R, R,
                                                     stride, pad, kw))
        for a, b in zip(call(0), call(1)):
            if not torch.equal(a, b):
                raise RuntimeError(f"{op} {name}: walk differs from decode")
        # 30 warm-up calls per variant: the first timed round must not be
        # the one in which the allocator and the clocks settle
        res = _time_alternating({kw: (lambda kw=kw: call(kw))
                                 for kw in (0, 1)}, rounds=rounds, warmup=30)
        for kw in (0, 1):
            med, lo, hi = res[kw]
            print(f"{op:6s} {name:8s} {kw:5d} {plan(kw):7s} {med:9.1f} "
                  f"{lo:9.1f} {hi:9.1f} {med / res[0][0]:9.3f} "
                  f"{flops / med / 1e6:8.1f}", flush=True)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--wgradbias", action="store_true")
    ap.add_argument("--wgraddma", action="store_true")
    ap.add_argument("--wgraddma-child", action="store_true",
                    help=argparse.SUPPRESS)
    ap.add_argument("--leaves", default="",
                    help="further DDPX_WGRAD_V letters for --wgraddma, "
                         "comma separated (e.g. wt3)")
    ap.add_argument("--dgradtaps", action="store_true")
    ap.add_argument("--groups", default="0,32,64,128",
                    help="conv2d_dgrad group values for --dgradtaps, raster "
                         "(0) first")
    ap.add_argument("--kwalk", action="store_true")
    ap.add_argument("--resnet", action="store_true")
    ap.add_argument("--functional", action="store_true")
    ap.add_argument("--bn", action="store_true")
    ap.add_argument("--bnpool", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if args.clip:
        bench_clip(rounds=30)
        return
    if args.wgradbias:
        bench_wgradbias(rounds=30)
        return
    if args.wgraddma_child:
        _wgraddma_child()
        return
    if args.wgraddma:
        bench_wgraddma(rounds=30, extra=args.leaves.split(","))
        return
    if args.dgradtaps:
        bench_dgradtaps(rounds=30,
                        groups=[int(v) for v in args.groups.split(",")])
        return
    if args.kwalk:
        bench_kwalk(rounds=30)
        return
    if args.bn:
        bench_bn(args.reps)
        return
    if args.bnpool:
        bench_bnpool(args.reps)
        return
    if args.functional:
        load_extension(required=True)
        bench_functional(TOYNET + (RESNET if args.resnet else []), args.reps)
        return
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    shapes = TOYNET + (RESNET if args.resnet else [])
    print(f"{'shape':8s} {'op':6s} {'us':>9s} {'TFLOP/s':>9s}")
    for name, N, C, H, W, K, R, stride, pad in shapes:
        P = (H + 2 * pad - R) // stride + 1
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(K, C, R, R, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, K, P, P, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
        wt2 = w.to(torch.bfloat16).permute(1, 2, 3, 0).reshape(C, R * R * K).contiguous()
        flops = 2.0 * N * P * P * K * C * R * R
        us = time_op(lambda: ext.conv2d_fwd(x, w, None, stride, pad), args.reps)
        print(f"{name:8s} {'fwd':6s} {us:9.1f} {flops/us/1e6:9.1f}")
        if C >= 8:
            us = time_op(lambda: ext.conv2d_dgrad(dy, wt2, N, C, H, W, R, R,
                                                  stride, pad), args.reps)
            print(f"{name:8s} {'dgrad':6s} {us:9.1f} {flops/us/1e6:9.1f}")
        us = time_op(lambda: ext.conv2d_wgrad(dy, x, R, R, stride, pad),
                     args.reps)
        print(f"{name:8s} {'wgrad':6s} {us:9.1f} {flops/us/1e6:9.1f}")


if __name__ == "__main__":
    main()
