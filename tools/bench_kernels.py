"""Micro-benchmark of the HIP conv kernels at the workload's shapes.

Usage (on a GPU box):  python tools/bench_kernels.py [--resnet]
                       python tools/bench_kernels.py --bn | --bnpool
                       python tools/bench_kernels.py --clip
                       python tools/bench_kernels.py --wgradbias
                       python tools/bench_kernels.py --wgraddma [--leaves wt3]
                       python tools/bench_kernels.py --dgradtaps
                       python tools/bench_kernels.py --kwalk
                       python tools/bench_kernels.py --wgradwalk
                       python tools/bench_kernels.py --stem
                       python tools/bench_kernels.py --linear
                       python tools/bench_kernels.py --dwconv [--trs 4,8,32]
                       python tools/bench_kernels.py --dwconvk [--tos 1,2,4]
                       python tools/bench_kernels.py --gconv
                       python tools/bench_kernels.py --gn | --se
                       python tools/bench_kernels.py --ln [--blocks 512,4096]
                       python tools/bench_kernels.py --attn

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


VGG_L3 = ("vgg256", 64, 256, 56, 56, 256, 3, 1, 1)


def bench_wgradwalk(rounds):
    """Tile loop of the wide wgrad leaves: per-tile row decode (walk 0)
    against carried rows (walk 1), alternated in one process (`walk` is an
    argument).  Toy_Net's conv2, conv3 and conv4 at B = 1024 go through
    conv2d_wgrad_bias as the training step calls them; r18s1 (not a wide
    leaf: both sides run decode, a control) and one VGG layer with pad 1 run
    without bias.  Three more rows complete the (DEPTH 64) x (bias) x (pad)
    classes the automatic plan decides on: conv3 and conv4 without bias, the
    VGG layer with bias.  dw (and db) are checked torch.equal before timing;
    30 warm-up calls, then device events around 10 calls, median/min/max over
    `rounds`."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    by_name = {s[0]: s for s in TOYNET + RESNET + [VGG_L3]}
    rows = [("conv2", True), ("conv3", True), ("conv4", True),
            ("r18s1", False), ("vgg256", False),
            ("conv3", False), ("conv4", False), ("vgg256", True)]
    print(f"{'shape':8s} {'bias':>4s} {'pad':>3s} {'leaf':13s} {'walk':>4s} "
          f"{'plan':7s} {'med us':>9s} {'min':>9s} {'max':>9s} "
          f"{'vs decode':>9s} {'TFLOP/s':>8s}")
    for name, bias in rows:
        _, N, C, H, W, K, R, stride, pad = by_name[name]
        P = (H + 2 * pad - R) // stride + 1
        flops = 2.0 * N * P * P * K * C * R * R
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(N, C, H, W, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, K, P, P, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        geom = (N, C, H, W, K, R, R, stride, pad, bias)
        leaf = ext.conv2d_wgrad_plan(*geom)[0]
        if bias:
            call = (lambda wk: ext.conv2d_wgrad_bias(dy, x, R, R, stride,
                                                     pad, wk))
        else:
            call = (lambda wk: [ext.conv2d_wgrad(dy, x, R, R, stride, pad,
                                                 wk)])
        for a, b in zip(call(0), call(1)):
            if a is not None and not torch.equal(a, b):
                raise RuntimeError(f"wgrad {name}: walk differs from decode")
        res = _time_alternating({wk: (lambda wk=wk: call(wk))
                                 for wk in (0, 1)}, rounds=rounds, warmup=30)
        for wk in (0, 1):
            med, lo, hi = res[wk]
            plan = ext.conv2d_wgrad_kloop_plan(*geom, wk)[0]
            print(f"{name:8s} {int(bias):4d} {pad:3d} {leaf:13s} {wk:4d} "
                  f"{plan:7s} {med:9.1f} {lo:9.1f} {hi:9.1f} "
                  f"{med / res[0][0]:9.3f} {flops / med / 1e6:8.1f}",
                  flush=True)
        del x, dy
        torch.cuda.empty_cache()


def bench_linear(rounds):
    """The linear layers' three products through their whole entry points
    (transposes and slab combines included): the legacy path (impl 0)
    against the LDS-DMA kernel (impl 1), alternated in one process (`impl`
    is an argument).  Shapes: Toy_Net's Linear(8192, 512) at B = 1024,
    VGG-16's Linear(25088, 4096) and Linear(4096, 4096) at B = 256.  Outputs
    are checked equal before timing; 30 warm-up calls, then device events
    around 10 calls, median/min/max over `rounds`."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    shapes = [("toy fc1", 1024, 512, 8192), ("vgg fc1", 256, 4096, 25088),
              ("vgg fc2", 256, 4096, 4096)]
    print(f"{'layer':8s} {'op':6s} {'impl':>4s} {'plan':7s} {'auto':7s} "
          f"{'med us':>9s} {'min':>9s} {'max':>9s} {'vs legacy':>9s} "
          f"{'TFLOP/s':>8s}")
    for name, M, N, K in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) / 64) \
            .to(torch.bfloat16)
        dy = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
        b = torch.randn(N, device=dev, generator=g)
        calls = [("fwd", 0, lambda i: ext.linear_fwd(x, w, b, i)),
                 ("dgrad", 1, lambda i: ext.linear_dgrad(dy, w, i)),
                 ("wgrad", 2, lambda i: ext.linear_wgrad(dy, x, i))]
        flops = 2.0 * M * N * K
        for op, code, call in calls:
            if not torch.equal(call(0), call(1)):
                raise RuntimeError(f"{name} {op}: dma differs from legacy")
            res = _time_alternating({i: (lambda i=i: call(i))
                                     for i in (0, 1)}, rounds=rounds,
                                    warmup=30)
            for i in (0, 1):
                med, lo, hi = res[i]
                print(f"{name:8s} {op:6s} {i:4d} "
                      f"{ext.linear_plan(code, M, N, K, i):7s} "
                      f"{ext.linear_plan(code, M, N, K):7s} {med:9.1f} "
                      f"{lo:9.1f} {hi:9.1f} {med / res[0][0]:9.3f} "
                      f"{flops / med / 1e6:8.1f}", flush=True)
        del x, w, dy
        torch.cuda.empty_cache()


def _wide_slab_rows(ext, rounds):
    """bn_fwd_train behind a conv-epilogue slab, one slice per 128-row
    M-tile: Toy_Net's BN1 (C = 64, S = 5408) and BN2 (C = 128, S = 4608) at
    B = 1024.  The call is the combine plus the apply pass."""
    dev = torch.device("cuda:0")
    print(f"{'op':14s} {'C':>4s} {'S':>5s} {'med us':>9s} {'min':>9s} "
          f"{'max':>9s}")
    for C, HW in ((64, 26), (128, 24)):
        M = 1024 * HW * HW
        S = (M + 127) // 128
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(1024, C, HW, HW, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        slab = torch.rand(2, C, S, device=dev, generator=g) * 128.0
        slab[1] += 128.0
        gamma = torch.ones(C, device=dev)
        beta = torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def call():
            return ext.bn_fwd_train(x, gamma, beta, rm, rv, 0.1, 1e-5, True,
                                    None, slab)
        res = _time_alternating({"bn": call}, rounds=rounds, warmup=30)
        med, lo, hi = res["bn"]
        print(f"{'bn_fwd_train':14s} {C:4d} {S:5d} {med:9.1f} {lo:9.1f} "
              f"{hi:9.1f}", flush=True)
        del x, slab
        torch.cuda.empty_cache()


def bench_stem(rounds):
    """Toy_Net's stem (1 -> 64 channels, 3x3, 28x28, B = 1024) through
    conv2d_stem_fwd with statistics: the MFMA path on channels padded to 8
    (stem 0: pad kernel, weight pack and implicit GEMM, what a training step
    launches) against the direct kernel (stem 1), alternated in one process
    (`stem` is an argument).  y and the float64 slab totals are checked
    against the MFMA path before timing; 30 warm-up calls, then device
    events around 10 calls, median/min/max over `rounds`.  GB/s is the
    88.6 MB y write over the median.  Then the wide-slab BN rows."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    N, C, H, W, K, R, stride, pad = 1024, 1, 28, 28, 64, 3, 1, 0
    P = H - 2
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(N, C, H, W, device=dev, generator=g) \
        .to(torch.bfloat16).contiguous(memory_format=CL)
    w = torch.randn(K, C, R, R, device=dev, generator=g) / 3.0
    b = torch.randn(K, device=dev, generator=g)

    def call(stem):
        return ext.conv2d_stem_fwd(x, w, b, stride, pad, True, stem)
    (y0, s0), (y1, s1) = call(0), call(1)
    # the two paths add the nine products in different orders: y may differ
    # by one bf16 ulp where v sits on a rounding boundary, nowhere by more
    d = (y1.float() - y0.float()).abs()
    ulp = y0.float().abs().clamp(min=2.0 ** -126) * 2.0 ** -7
    if not bool((d <= ulp).all()):
        raise RuntimeError("stem: direct differs from mfma by more than "
                           "one bf16 ulp")
    t0, t1 = s0.double().sum(2), s1.double().sum(2)
    if not torch.allclose(t1, t0, rtol=1e-4, atol=1e-2):
        raise RuntimeError("stem: slab totals differ")
    print(f"y: {float((d > 0).float().mean()) * 100:.3f} % of elements differ "
          f"(each by one bf16 ulp at most); slab totals agree to 1e-4")
    ybytes = N * P * P * K * 2
    print(f"{'stem':>4s} {'plan':7s} {'med us':>9s} {'min':>9s} {'max':>9s} "
          f"{'vs mfma':>8s} {'y GB/s':>8s}")
    res = _time_alternating({st: (lambda st=st: call(st)) for st in (0, 1)},
                            rounds=rounds, warmup=30)
    for st in (0, 1):
        med, lo, hi = res[st]
        plan = ext.conv2d_stem_plan(N, C, H, W, K, R, R, stride, pad, st)
        print(f"{st:4d} {plan:7s} {med:9.1f} {lo:9.1f} {hi:9.1f} "
              f"{med / res[0][0]:8.3f} {ybytes / med / 1e3:8.0f}", flush=True)
    del x, y0, y1
    torch.cuda.empty_cache()
    _wide_slab_rows(ext, rounds)


# the nine distinct MobileNetV1 depthwise shapes (C, H = W, stride), pad 1
DWCONV = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2),
          (256, 28, 1), (256, 28, 2), (512, 14, 1), (512, 14, 2),
          (1024, 7, 1)]
HBM_PEAK = 8.0e12      # bytes/s, MI355X HBM3E


def bench_dwconv(rounds, trs):
    """Depthwise 3x3 kernels (dwconv.hip) at B = 256 on MobileNetV1's shapes
    against torch's own kernels for F.conv2d(groups=C) in bf16 channels_last
    (aten convolution / convolution_backward with one output mask bit each),
    alternated in one process.  Each row: median us of our kernel (min-max),
    GB/s on the minimum bytes the op must move (every operand read once,
    every result written once; the fp32 slabs not counted), that minimum over
    the 8 TB/s HBM peak as a share of the measured time, torch's median and
    torch / ours.  Outputs are compared with torch's before timing.  `trs`:
    further strip heights timed for the forward (the plan's choice is -1)."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    N, pad = 256, 1
    aten = torch.ops.aten
    print(f"{'C':>5s} {'H':>4s} {'s':>2s} {'op':10s} {'med us':>8s} "
          f"{'min':>8s} {'max':>8s} {'GB/s':>7s} {'%HBM':>6s} "
          f"{'torch us':>9s} {'torch/ours':>10s}")
    for C, H, stride in DWCONV:
        g = torch.Generator(device=dev).manual_seed(C + H + stride)
        P = (H + 2 * pad - 3) // stride + 1
        x = torch.randn(N, C, H, H, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, C, P, P, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(C, 1, 3, 3, device=dev, generator=g) / 3.0
        wb = w.to(torch.bfloat16).contiguous(memory_format=CL)
        xb, yb = x.numel() * 2, dy.numel() * 2

        def t_bwd(mask):
            return aten.convolution_backward(
                dy, x, wb, None, [stride] * 2, [pad] * 2, [1, 1], False,
                [0, 0], C, mask)
        ops = {
            "fwd": (lambda tr=-1: ext.dwconv2d_fwd(x, w, None, stride, pad,
                                                   False, tr)[0],
                    lambda: torch.nn.functional.conv2d(
                        x, wb, None, stride, pad, 1, C), xb + yb),
            "fwd+stats": (lambda: ext.dwconv2d_fwd(x, w, None, stride, pad,
                                                   True)[0],
                          None, xb + yb),
            "dgrad": (lambda: ext.dwconv2d_dgrad(dy, w, H, H, stride, pad),
                      lambda: t_bwd([True, False, False])[0], xb + yb),
            "wgrad": (lambda: ext.dwconv2d_wgrad(dy, x, stride, pad,
                                                 False)[0],
                      lambda: t_bwd([False, True, False])[1].float(),
                      xb + yb),
        }
        for name, (ours, theirs, nbytes) in ops.items():
            variants = {"ours": ours}
            if theirs is not None:
                a, b = ours().float(), theirs().float()
                err = float((a - b).abs().max() / b.abs().max())
                # torch's results are bf16 (its wgrad too): one bf16 ulp of
                # the largest element is 2^-7 of it
                if err > 2.0 ** -5:
                    raise RuntimeError(f"dwconv {name} C{C} H{H} s{stride}: "
                                       f"differs from torch by {err:.3g}")
                variants["torch"] = theirs
            if name == "fwd":
                for tr in trs:
                    variants[f"tr{tr}"] = (lambda tr=tr: ours(tr))
            res = _time_alternating(variants, rounds=rounds, warmup=10)
            med, lo, hi = res["ours"]
            tm = res["torch"][0] if "torch" in res else float("nan")
            print(f"{C:5d} {H:4d} {stride:2d} {name:10s} {med:8.1f} {lo:8.1f} "
                  f"{hi:8.1f} {nbytes / med / 1e3:7.0f} "
                  f"{nbytes / HBM_PEAK * 1e6 / med * 100:6.1f} {tm:9.1f} "
                  f"{tm / med:10.2f}", flush=True)
            for tr in (trs if name == "fwd" else ()):
                m2 = res[f"tr{tr}"]
                print(f"{'':12s} fwd tr={tr:<3d} {m2[0]:8.1f} {m2[1]:8.1f} "
                      f"{m2[2]:8.1f}", flush=True)
        del x, dy
        torch.cuda.empty_cache()


# (K, C, H, stride): MnasNet-B1's six 5x5 depthwise shapes, then 7x7 stride 1
DWCONVK = [(5, 72, 56, 2), (5, 120, 28, 1), (5, 240, 28, 2), (5, 480, 14, 1),
           (5, 576, 14, 2), (5, 1152, 7, 1),
           (7, 96, 56, 1), (7, 192, 28, 1), (7, 384, 14, 1), (7, 768, 7, 1)]


def bench_dwconvk(rounds, tos):
    """Depthwise 5x5 / 7x7 kernels (dwconvk.hip) at B = 256, pad K // 2,
    against torch's own kernels for F.conv2d(groups=C) in bf16 channels_last
    (aten convolution / convolution_backward with one output mask bit each),
    alternated in one process: 30 warm-up calls, device events around 10
    calls, median of `rounds` rounds with min-max.  %HBM is the time the op's
    two activation tensors take once each at 8 TB/s (x + y forward, dy + dx
    dgrad, dy + x wgrad) as a share of the measured time.  Outputs are
    compared with torch's before timing.  `tos`: further run heights timed
    for the forward (the plan's choice is -1)."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    N = 256
    aten = torch.ops.aten
    print(f"{'K':>2s} {'C':>5s} {'H':>4s} {'s':>2s} {'op':10s} {'med us':>8s} "
          f"{'min':>8s} {'max':>8s} {'GB/s':>7s} {'%HBM':>6s} "
          f"{'torch us':>9s} {'torch/ours':>10s}")
    for K, C, H, stride in DWCONVK:
        pad = K // 2
        g = torch.Generator(device=dev).manual_seed(K + C + H + stride)
        P = (H + 2 * pad - K) // stride + 1
        x = torch.randn(N, C, H, H, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, C, P, P, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(C, 1, K, K, device=dev, generator=g) / K
        wb = w.to(torch.bfloat16).contiguous(memory_format=CL)
        nbytes = (x.numel() + dy.numel()) * 2

        def t_bwd(mask):
            return aten.convolution_backward(
                dy, x, wb, None, [stride] * 2, [pad] * 2, [1, 1], False,
                [0, 0], C, mask)
        ops = {
            "fwd": (lambda to=-1: ext.dwconvk2d_fwd(x, w, None, stride, pad,
                                                    False, to)[0],
                    lambda: torch.nn.functional.conv2d(
                        x, wb, None, stride, pad, 1, C)),
            "fwd+stats": (lambda: ext.dwconvk2d_fwd(x, w, None, stride, pad,
                                                    True)[0], None),
            "dgrad": (lambda: ext.dwconvk2d_dgrad(dy, w, H, H, stride, pad),
                      lambda: t_bwd([True, False, False])[0]),
            "wgrad": (lambda: ext.dwconvk2d_wgrad(dy, x, K, stride, pad,
                                                  False)[0],
                      lambda: t_bwd([False, True, False])[1].float()),
        }
        for name, (ours, theirs) in ops.items():
            variants = {"ours": ours}
            if theirs is not None:
                a, b = ours().float(), theirs().float()
                err = float((a - b).abs().max() / b.abs().max())
                # torch's results are bf16 (its wgrad too): one bf16 ulp of
                # the largest element is 2^-7 of it
                if err > 2.0 ** -5:
                    raise RuntimeError(f"dwconvk {name} K{K} C{C} H{H} "
                                       f"s{stride}: differs from torch by "
                                       f"{err:.3g}")
                variants["torch"] = theirs
            if name == "fwd":
                for to in tos:
                    variants[f"to{to}"] = (lambda to=to: ours(to))
            res = _time_alternating(variants, rounds=rounds, warmup=30)
            med, lo, hi = res["ours"]
            tm = res["torch"][0] if "torch" in res else float("nan")
            print(f"{K:2d} {C:5d} {H:4d} {stride:2d} {name:10s} {med:8.1f} "
                  f"{lo:8.1f} {hi:8.1f} {nbytes / med / 1e3:7.0f} "
                  f"{nbytes / HBM_PEAK * 1e6 / med * 100:6.1f} {tm:9.1f} "
                  f"{tm / med:10.2f}", flush=True)
            for to in (tos if name == "fwd" else ()):
                m2 = res[f"to{to}"]
                print(f"{'':15s} fwd to={to:<3d} {m2[0]:8.1f} {m2[1]:8.1f} "
                      f"{m2[2]:8.1f}", flush=True)
        del x, dy
        torch.cuda.empty_cache()


# ResNeXt-50 32x4d's grouped convs (C, H, stride, Cg) and a Cg = 64 layer
GCONV = [(128, 56, 1, 4), (256, 56, 2, 8), (256, 28, 1, 8), (512, 28, 2, 16),
         (512, 14, 1, 16), (1024, 14, 2, 32), (1024, 7, 1, 32),
         (2048, 7, 1, 64)]


def bench_gconv(rounds):
    """Grouped 3x3 kernels (gconv.hip) at B = 256, pad 1, against (a) torch's
    own kernels for F.conv2d(groups=) / convolution_backward in bf16
    channels_last and (b), forward only, this project's dense path on the
    block-diagonally expanded weight; alternated in one process, 30 warm-up
    calls, device events around 10 calls.  Each row: median us (min-max), the
    share of the HBM-bound time (the two activation tensors the op must move,
    once each, at 8 TB/s: x and y forward, dy and dx dgrad, dy and x wgrad),
    the comparisons' medians and their ratio to ours.  Outputs are compared
    with torch's before timing."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    N, pad = 256, 1
    aten = torch.ops.aten
    print(f"{'C':>5s} {'H':>4s} {'s':>2s} {'Cg':>3s} {'op':6s} {'med us':>8s} "
          f"{'min':>8s} {'max':>8s} {'%HBM':>6s} {'bound':>6s} "
          f"{'torch us':>9s} {'torch/ours':>10s} {'dense us':>9s} "
          f"{'dense/ours':>10s}")
    for C, H, stride, Cg in GCONV:
        groups = C // Cg
        g = torch.Generator(device=dev).manual_seed(C + H + stride)
        P = (H + 2 * pad - 3) // stride + 1
        x = torch.randn(N, C, H, H, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(N, C, P, P, device=dev, generator=g) \
            .to(torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(C, Cg, 3, 3, device=dev, generator=g) / 3.0
        wb = w.to(torch.bfloat16).contiguous(memory_format=CL)
        img, img_t = ext.gconv2d_pack(w)
        wd = torch.zeros(C, C, 3, 3, device=dev)
        for k in range(groups):
            wd[k * Cg:(k + 1) * Cg, k * Cg:(k + 1) * Cg] = \
                w[k * Cg:(k + 1) * Cg]
        wdb = wd.to(torch.bfloat16).contiguous(memory_format=CL)
        del wd
        xb, yb = x.numel() * 2, dy.numel() * 2

        def t_bwd(mask):
            return aten.convolution_backward(
                dy, x, wb, None, [stride] * 2, [pad] * 2, [1, 1], False,
                [0, 0], groups, mask)
        ops = {
            "fwd": (lambda: ext.gconv2d_fwd(x, img, None, groups, stride, pad,
                                            False)[0],
                    lambda: torch.nn.functional.conv2d(
                        x, wb, None, stride, pad, 1, groups),
                    lambda: ext.conv2d_fwd(x, wdb, None, stride, pad),
                    "x+y"),
            "dgrad": (lambda: ext.gconv2d_dgrad(dy, img_t, H, H, groups,
                                                stride, pad),
                      lambda: t_bwd([True, False, False])[0], None, "dy+dx"),
            "wgrad": (lambda: ext.gconv2d_wgrad(dy, x, groups, stride, pad),
                      lambda: t_bwd([False, True, False])[1].float(), None,
                      "dy+x"),
        }
        for name, (ours, theirs, dense, bound) in ops.items():
            variants = {"ours": ours, "torch": theirs}
            if dense is not None:
                variants["dense"] = dense
            a = ours().float()
            for other in list(variants)[1:]:
                b = variants[other]().float()
                err = float((a - b).abs().max() / b.abs().max())
                # torch's results are bf16 (its wgrad too): one bf16 ulp of
                # the largest element is 2^-7 of it
                if err > 2.0 ** -5:
                    raise RuntimeError(f"gconv {name} C{C} H{H} s{stride}: "
                                       f"differs from {other} by {err:.3g}")
            res = _time_alternating(variants, rounds=rounds, warmup=30)
            med, lo, hi = res["ours"]
            tm = res["torch"][0]
            dm = res["dense"][0] if dense is not None else float("nan")
            print(f"{C:5d} {H:4d} {stride:2d} {Cg:3d} {name:6s} {med:8.1f} "
                  f"{lo:8.1f} {hi:8.1f} "
                  f"{(xb + yb) / HBM_PEAK * 1e6 / med * 100:6.1f} {bound:>6s} "
                  f"{tm:9.1f} {tm / med:10.2f} {dm:9.1f} {dm / med:10.2f}",
                  flush=True)
        del x, dy
        torch.cuda.empty_cache()


# ResNet-50 norm shapes (C, H) for --gn
GN_SHAPES = [(64, 112), (256, 56), (512, 28), (1024, 14), (2048, 7)]


def bench_gn(rounds):
    """GroupNorm kernels (gn.hip), G = 32, relu + residual, at B = 32 and 256,
    forward and backward apart, against (a) torch's F.group_norm + add + relu
    (its autograd for the backward) on the same bf16 channels_last tensors and
    (b) this project's bn_fwd_train / bn_bwd at the same shape; alternated in
    one process, 30 warm-up calls, device events around 10 calls.  Each row:
    median us (min-max), the share of the HBM-bound time of the least traffic
    at 8 TB/s (forward: x twice + y; backward: x and dy twice + dx; residual,
    dresid and mask not counted), the comparisons' medians and their ratio to
    ours, and the size of x: a share above 100 % can only come from second
    reads served by the Infinity Cache (256 MiB).  Every output is checked
    against torch's fp32 formula before timing."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    G, eps = 32, 1e-5
    Fn = torch.nn.functional
    print(f"{'B':>4s} {'C':>5s} {'H':>4s} {'op':4s} {'med us':>8s} {'min':>8s} "
          f"{'max':>8s} {'%HBM':>6s} {'torch us':>9s} {'torch/ours':>10s} "
          f"{'bn us':>8s} {'ours/bn':>8s} {'x MiB':>7s}")
    for N in (32, 256):
        for C, H in GN_SHAPES:
            g = torch.Generator(device=dev).manual_seed(N + C + H)

            def act():
                return (torch.randn(N, C, H, H, device=dev, generator=g)
                        .to(torch.bfloat16).contiguous(memory_format=CL))
            x, r, dy = act() * 1.5 + 0.5, act(), act()
            gam = torch.rand(C, device=dev, generator=g) + 0.5
            bet = torch.rand(C, device=dev, generator=g) - 0.5
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            y, mean, invstd, mask = ext.gn_fwd(x, gam, bet, G, eps, True, r)
            _, bm, bi, bmask = ext.bn_fwd_train(x, gam, bet, rm, rv, 0.1, eps,
                                                True, r, None)
            xt, rt = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
            gt, bt = (gam.bfloat16().requires_grad_(True),
                      bet.bfloat16().requires_grad_(True))

            def t_fwd():
                return Fn.relu(Fn.group_norm(xt, G, gt, bt, eps) + rt)
            yt = t_fwd()

            def t_bwd():
                return torch.autograd.grad(yt, (xt, gt, bt, rt), dy,
                                           retain_graph=True)
            ours_b = ext.gn_bwd(x, dy, gam, mean, invstd, mask, G, True, True)
            # every output, max error: y and dx against torch's fp32 formula
            # on the GPU to a bf16 ulp (2^-8 of the element, plus 2^-12 of
            # the largest for the fp32 sums on either side), dgamma and
            # dbeta against float64 sums to 2^-10 of the largest, the mask
            # wherever |v| > 2^-10, dresid exactly.  The reference backward takes our mask as
            # dy_eff: torch's own bf16 path rounds norm(x) before its relu
            # and flips borderline bits.
            xf = x.float().requires_grad_(True)
            gf, bf = gam.clone().requires_grad_(True), \
                bet.clone().requires_grad_(True)
            v = Fn.group_norm(xf, G, gf, bf, eps) + r.float()
            bits = ((mask.view(N, H, H, C // 8, 1) >> torch.arange(
                8, device=dev, dtype=torch.uint8)) & 1).bool() \
                .reshape(N, H, H, C).permute(0, 3, 1, 2)
            ge = dy.float() * bits
            refs = list(torch.autograd.grad(v, (xf, gf, bf), ge))
            v = v.detach()
            # dgamma, dbeta: float64 sums (torch's fp32 ones drift at B = 256)
            xg = x.double().reshape(N, G, -1)
            xh = ((xg - xg.mean(2, keepdim=True))
                  / (xg.var(2, unbiased=False, keepdim=True) + eps).sqrt())
            refs[1] = (ge.double() * xh.reshape(N, C, H, H)).sum((0, 2, 3))
            refs[2] = ge.double().sum((0, 2, 3))
            del xg, xh
            live = v.abs() > 2.0 ** -10
            checks = [("mask", bits[live] == (v > 0)[live], None, 0),
                      ("dresid", ours_b[3].float(), ge, 0),
                      ("y", y.float(), v.clamp_min(0), 2.0 ** -8),
                      ("dx", ours_b[0].float(), refs[0], 2.0 ** -8),
                      ("dgamma", ours_b[1].double(), refs[1], 0),
                      ("dbeta", ours_b[2].double(), refs[2], 0)]
            for name, got, ref, rel in checks:
                if ref is None:
                    ok = bool(got.all())
                elif name == "dresid":
                    ok = torch.equal(got, ref)
                else:
                    slack = ref.abs().max() * (2.0 ** -12 if rel else
                                               2.0 ** -10)
                    ok = bool(((got - ref).abs()
                               <= rel * ref.abs() + slack).all())
                if not ok:
                    raise RuntimeError(f"gn {name} B{N} C{C} H{H} differs "
                                       "from the fp32 reference")
            del xf, v, bits, ge, refs, live, checks
            xb = x.numel() * 2
            ops = {
                "fwd": (lambda: ext.gn_fwd(x, gam, bet, G, eps, True, r),
                        lambda: t_fwd(),
                        lambda: ext.bn_fwd_train(x, gam, bet, rm, rv, 0.1, eps,
                                                 True, r, None), 3 * xb),
                "bwd": (lambda: ext.gn_bwd(x, dy, gam, mean, invstd, mask, G,
                                           True, True),
                        t_bwd,
                        lambda: ext.bn_bwd(x, dy, gam, bm, bi, bmask, True,
                                           True, None, False), 5 * xb),
            }
            for name, (ours, theirs, bn, traffic) in ops.items():
                res = _time_alternating({"ours": ours, "torch": theirs,
                                         "bn": bn}, rounds=rounds, warmup=30)
                med, lo, hi = res["ours"]
                tm, bnm = res["torch"][0], res["bn"][0]
                print(f"{N:4d} {C:5d} {H:4d} {name:4s} {med:8.1f} {lo:8.1f} "
                      f"{hi:8.1f} {traffic / HBM_PEAK * 1e6 / med * 100:6.1f} "
                      f"{tm:9.1f} {tm / med:10.2f} {bnm:8.1f} "
                      f"{med / bnm:8.2f} {xb / 2 ** 20:7.1f}", flush=True)
            del x, r, dy, y, yt, xt, rt, ours_b, mask, bmask
            torch.cuda.empty_cache()


# SE-ResNeXt-50 junction shapes (C, H) for --se
SE_SHAPES = [(256, 56), (512, 28), (1024, 14), (2048, 7)]


def bench_se(rounds):
    """The Squeeze-and-Excitation junction (se.hip + the linear kernels),
    r = 16, relu + residual, at B = 32 and 256: forward and backward of the
    whole autograd Function against the torch composition (adaptive avg-pool,
    two F.linear, sigmoid, mul, add, relu, and its autograd) on the same bf16
    channels_last tensors and bf16 weights; alternated in one process, 30
    warm-up calls, device events around 10 calls.  Each row: median us
    (min-max), the share of the HBM-bound time of the least traffic at 8 TB/s
    (forward 2u + r + y, backward 2dy + 2u + dx + dresid; mask and the [N, C]
    tensors not counted), torch's median and its ratio to ours, the size of u.
    Before timing y is checked against the fp32 formula, and dx, dresid and
    the four parameter gradients against the fp32 formula's autograd with
    this path's mask as dy_eff."""
    from ddp_tricks_amd.ops import SqueezeExcite
    dev = torch.device("cuda:0")
    Fn = torch.nn.functional
    print(f"{'B':>4s} {'C':>5s} {'H':>4s} {'op':4s} {'med us':>8s} {'min':>8s} "
          f"{'max':>8s} {'%HBM':>6s} {'torch us':>9s} {'torch/ours':>10s} "
          f"{'u MiB':>7s}")
    for N in (32, 256):
        for C, H in SE_SHAPES:
            g = torch.Generator(device=dev).manual_seed(N + C + H)

            def act():
                return (torch.randn(N, C, H, H, device=dev, generator=g)
                        .to(torch.bfloat16).contiguous(memory_format=CL))
            u, r, dy = act().requires_grad_(True), act().requires_grad_(True), act()
            se = SqueezeExcite(C, 16).to(dev)
            with torch.no_grad():   # hidden units clear of the relu's edge:
                # a unit whose sign differs between two roundings of z flips
                # its whole gradient row, in any implementation
                se.fc1.bias.copy_(1.0 - 2.0 * (torch.arange(C // 16) % 2))
            ps = list(se.parameters())
            wt = [p.detach().flatten(1).bfloat16().requires_grad_(True)
                  if p.dim() == 4 else p.detach().bfloat16().requires_grad_(True)
                  for p in ps]

            def ours_fwd():
                return se(u, residual=r, fuse_relu=True)

            def t_fwd(x=u, res=r, w=wt, relu=True):
                z = Fn.adaptive_avg_pool2d(x, 1).flatten(1)
                s = torch.sigmoid(Fn.linear(Fn.relu(Fn.linear(z, w[0], w[1])),
                                            w[2], w[3]))
                v = x * s[:, :, None, None] + res
                return Fn.relu(v) if relu else v
            y, yt = ours_fwd(), t_fwd()

            def ours_bwd():
                return torch.autograd.grad(y, [u, r] + ps, dy,
                                           retain_graph=True)

            def t_bwd():
                return torch.autograd.grad(yt, [u, r] + wt, dy,
                                           retain_graph=True)
            # fp32 formula over the bf16-rounded operands, without its relu:
            # the backward takes dy where OUR output is positive (borderline
            # relu bits differ between any two roundings of the gate)
            uf, rf = u.detach().float().requires_grad_(True), r.detach().float()
            wf = [w.detach().float().requires_grad_(True) for w in wt]
            v = t_fwd(uf, rf, wf, relu=False)
            ge = dy.float() * (y > 0)
            refs = torch.autograd.grad(v, [uf] + wf, ge)
            got = ours_bwd()
            checks = [("y", y.float(), v.detach().clamp_min(0)), ("dx", got[0].float(), refs[0]),
                      ("dresid", got[1].float(), ge)]
            checks += [(f"dparam{i}", got[2 + i].flatten(1).float()
                        if got[2 + i].dim() == 4 else got[2 + i].float(),
                        refs[1 + i]) for i in range(4)]
            for name, a, b in checks:
                # a bf16 ulp of the element plus 2^-6 of the largest: the
                # gate's bf16 roundings at z, h, a reach every output
                tol = 2.0 ** -7 * b.abs() + 2.0 ** -6 * b.abs().max()
                if not bool(((a - b).abs() <= tol).all()):
                    raise RuntimeError(
                        f"se {name} B{N} C{C} H{H} differs from the fp32 "
                        f"reference: largest error {(a - b).abs().max():.3g} "
                        f"of largest value {b.abs().max():.3g}")
            del uf, rf, wf, v, ge, refs, got, checks
            ub = u.numel() * 2
            for name, ours, theirs, traffic in (
                    ("fwd", ours_fwd, t_fwd, 4 * ub),
                    ("bwd", ours_bwd, t_bwd, 6 * ub)):
                res = _time_alternating({"ours": ours, "torch": theirs},
                                        rounds=rounds, warmup=30)
                med, lo, hi = res["ours"]
                tm = res["torch"][0]
                print(f"{N:4d} {C:5d} {H:4d} {name:4s} {med:8.1f} {lo:8.1f} "
                      f"{hi:8.1f} {traffic / HBM_PEAK * 1e6 / med * 100:6.1f} "
                      f"{tm:9.1f} {tm / med:10.2f} {ub / 2 ** 20:7.1f}",
                      flush=True)
            del u, r, dy, y, yt, se, ps, wt
            torch.cuda.empty_cache()


# ConvNeXt-T stages (C, H) for --ln
LN_SHAPES = [(96, 56), (192, 28), (384, 14), (768, 7)]


def bench_ln(rounds, blocks):
    """LayerNorm over C, GELU and layer scale (ln.hip) at B = 256 on
    ConvNeXt-T's four stages, the bindings against torch on the same bf16
    tensors: F.layer_norm over the permuted (NHWC-shaped) view and its
    autograd, F.gelu on the 4C-wide tensor and its autograd, resid + gamma * u
    and its autograd.  Alternated in one process, 30 warm-up calls, device
    events around 10 calls.  Each row: median us (min-max), the share of the
    HBM-bound time of the least traffic at 8 TB/s (activation tensors only:
    ln fwd x + y, bwd x + dy + dx; gelu fwd 2, bwd 3 tensors; layer scale fwd
    u + resid + y, bwd dy + u + du), torch's median and its ratio to ours.
    `blocks` adds LayerNorm forward / backward rows at forced grids.  Outputs
    are first compared with the fp32 formulas."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    Fn = torch.nn.functional
    N = 256
    print(f"{'C':>5s} {'H':>4s} {'op':12s} {'med us':>8s} {'min':>8s} "
          f"{'max':>8s} {'%HBM':>6s} {'torch us':>9s} {'torch/ours':>10s} "
          f"{'MiB':>7s}")

    def check(name, a, b):
        # a bf16 ulp of the element plus 2^-8 of the largest value
        tol = 2.0 ** -7 * b.abs() + 2.0 ** -8 * b.abs().max()
        if not bool(((a.float() - b).abs() <= tol).all()):
            raise RuntimeError(f"ln {name} differs from the fp32 reference: "
                               f"largest error {(a.float() - b).abs().max():.3g}")

    def row(C, H, name, ours, theirs, traffic, nbytes):
        res = _time_alternating({"ours": ours, "torch": theirs},
                                rounds=rounds, warmup=30)
        med, lo, hi = res["ours"]
        tm = res["torch"][0]
        print(f"{C:5d} {H:4d} {name:12s} {med:8.1f} {lo:8.1f} {hi:8.1f} "
              f"{traffic / HBM_PEAK * 1e6 / med * 100:6.1f} {tm:9.1f} "
              f"{tm / med:10.2f} {nbytes / 2 ** 20:7.1f}", flush=True)

    for C, H in LN_SHAPES:
        g = torch.Generator(device=dev).manual_seed(C + H)

        def act(c):
            return (torch.randn(N, c, H, H, device=dev, generator=g)
                    .to(torch.bfloat16).contiguous(memory_format=CL))
        x, r, dy = act(C), act(C), act(C)
        w = 1 + 0.5 * torch.randn(C, device=dev, generator=g)
        b = 0.5 * torch.randn(C, device=dev, generator=g)
        wb, bb = (t.bfloat16().requires_grad_(True) for t in (w, b))
        nb = x.numel() * 2

        # ---- LayerNorm
        xt = x.permute(0, 2, 3, 1).requires_grad_(True)
        dyt = dy.permute(0, 2, 3, 1)
        yt = Fn.layer_norm(xt, (C,), wb, bb, 1e-6)
        y, mean, rstd = ext.ln2d_fwd(x, w, b, 1e-6, True)
        xf = xt.detach().float().requires_grad_(True)
        wf, bf = (t.clone().requires_grad_(True) for t in (w, b))
        yf = Fn.layer_norm(xf, (C,), wf, bf, 1e-6)
        refs = torch.autograd.grad(yf, [xf, wf, bf], dyt.float())
        got = ext.ln2d_bwd(x, dy, w, mean, rstd)
        check("y", y.permute(0, 2, 3, 1), yf.detach())
        check("dx", got[0].permute(0, 2, 3, 1), refs[0])
        check("dgamma", got[1], refs[1])
        check("dbeta", got[2], refs[2])
        del xf, yf, refs, got
        row(C, H, "ln fwd", lambda: ext.ln2d_fwd(x, w, b, 1e-6, True),
            lambda: Fn.layer_norm(xt, (C,), wb, bb, 1e-6), 2 * nb, nb)
        row(C, H, "ln bwd", lambda: ext.ln2d_bwd(x, dy, w, mean, rstd),
            lambda: torch.autograd.grad(yt, [xt, wb, bb], dyt,
                                        retain_graph=True), 3 * nb, nb)
        for k in blocks:
            row(C, H, f"ln fwd b{k}",
                lambda: ext.ln2d_fwd(x, w, b, 1e-6, True, k),
                lambda: Fn.layer_norm(xt, (C,), wb, bb, 1e-6), 2 * nb, nb)
            row(C, H, f"ln bwd b{k}",
                lambda: ext.ln2d_bwd(x, dy, w, mean, rstd, k),
                lambda: torch.autograd.grad(yt, [xt, wb, bb], dyt,
                                            retain_graph=True), 3 * nb, nb)
        del xt, yt, y, mean, rstd

        # ---- layer scale
        ut, rt = x.detach().requires_grad_(True), r.detach().requires_grad_(True)
        st = wb.view(1, -1, 1, 1) * ut + rt
        uf, rf = x.float().requires_grad_(True), r.float().requires_grad_(True)
        sf = wf.view(1, -1, 1, 1) * uf + rf
        refs = torch.autograd.grad(sf, [uf, wf], dy.float())
        du, dgam = ext.lscale_bwd(dy, x, w)
        check("lscale y", ext.lscale_fwd(x, w, r), sf.detach())
        check("lscale du", du, refs[0])
        check("lscale dgamma", dgam, refs[1])
        del uf, rf, sf, refs, du, dgam
        row(C, H, "lscale fwd", lambda: ext.lscale_fwd(x, w, r),
            lambda: wb.view(1, -1, 1, 1) * ut + rt, 3 * nb, nb)
        row(C, H, "lscale bwd", lambda: ext.lscale_bwd(dy, x, w),
            lambda: torch.autograd.grad(st, [ut, rt, wb], dy,
                                        retain_graph=True), 3 * nb, nb)
        del ut, rt, st, x, r, dy

        # ---- GELU on the 4C-wide hidden tensor
        z, dz = act(4 * C), act(4 * C)
        zt = z.detach().requires_grad_(True)
        at_ = Fn.gelu(zt)
        zf = z.float().requires_grad_(True)
        af = Fn.gelu(zf)
        check("gelu a", ext.gelu_fwd(z), af.detach())
        check("gelu dz", ext.gelu_bwd(dz, z),
              torch.autograd.grad(af, zf, dz.float())[0])
        del zf, af
        row(4 * C, H, "gelu fwd", lambda: ext.gelu_fwd(z),
            lambda: Fn.gelu(zt), 2 * 4 * nb, 4 * nb)
        row(4 * C, H, "gelu bwd", lambda: ext.gelu_bwd(dz, z),
            lambda: torch.autograd.grad(at_, zt, dz, retain_graph=True),
            3 * 4 * nb, 4 * nb)
        del z, dz, zt, at_
        torch.cuda.empty_cache()


def bench_attn(rounds):
    """Attention forward, forward with lse saved, and backward (both kernels)
    of attn.hip at B = 256, heads 3 / 6 / 12, L = 64 / 196, against torch's
    F.scaled_dot_product_attention and its autograd on bf16 [N, heads, L, 64]
    tensors that torch is handed already permuted.  Alternated in one process,
    30 warm-up calls, device events around 10 calls.  Each row: median us
    (min-max), torch's median and its ratio to ours, achieved TFLOP/s (forward
    4 N heads L^2 64, backward the 7 tile GEMMs run: 14 N heads L^2 64) and the
    share of the HBM time of qkv + o (backward: qkv, o, do, dqkv) at 8 TB/s.
    Outputs are first compared with the fp32 formulas."""
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    Fn = torch.nn.functional
    N = 256
    print(f"{'heads':>5s} {'L':>4s} {'op':9s} {'med us':>8s} {'min':>8s} "
          f"{'max':>8s} {'torch us':>9s} {'torch/ours':>10s} {'TFLOP/s':>8s} "
          f"{'%HBM':>6s}")

    def check(name, a, b):
        tol = 2.0 ** -7 * b.abs() + 2.0 ** -8 * b.abs().max()
        if not bool(((a.float() - b).abs() <= tol).all()):
            raise RuntimeError(f"attn {name} differs from the fp32 reference: "
                               f"largest error {(a.float() - b).abs().max():.3g}")

    def heads_view(t, h):
        n, _, hh, ww = t.shape
        return t.permute(0, 2, 3, 1).reshape(n, hh * ww, h, 64).transpose(1, 2)

    for h in (3, 6, 12):
        for H in (8, 14):
            L, D = H * H, 64 * h
            g = torch.Generator(device=dev).manual_seed(h + H)
            qkv = (torch.randn(N, 3 * D, H, H, device=dev, generator=g)
                   .to(torch.bfloat16).contiguous(memory_format=CL))
            do = (torch.randn(N, D, H, H, device=dev, generator=g)
                  .to(torch.bfloat16).contiguous(memory_format=CL))
            qt, kt, vt = (heads_view(t, h).contiguous().requires_grad_(True)
                          for t in qkv.chunk(3, 1))
            dot = heads_view(do, h).contiguous()
            ot = Fn.scaled_dot_product_attention(qt, kt, vt)

            qf, kf, vf = (t.detach().float().requires_grad_(True)
                          for t in (qt, kt, vt))
            of = torch.softmax(qf @ kf.mT * 0.125, -1) @ vf
            refs = torch.autograd.grad(of, [qf, kf, vf], dot.float())
            o, lse = ext.attn_fwd(qkv, h, True)
            dqkv = ext.attn_bwd(qkv, o, lse, do, h)
            check("o", heads_view(o, h), of.detach())
            for name, got, ref in zip(("dq", "dk", "dv"), dqkv.chunk(3, 1),
                                      refs):
                check(name, heads_view(got, h), ref)
            del qf, kf, vf, of, refs, dqkv

            gemm = 2.0 * N * h * L * L * 64
            io = (qkv.numel() + o.numel()) * 2

            def row(name, ours, theirs, flops, traffic):
                res = _time_alternating({"ours": ours, "torch": theirs},
                                        rounds=rounds, warmup=30)
                med, lo, hi = res["ours"]
                tm = res["torch"][0]
                print(f"{h:5d} {L:4d} {name:9s} {med:8.1f} {lo:8.1f} "
                      f"{hi:8.1f} {tm:9.1f} {tm / med:10.2f} "
                      f"{flops / med / 1e6:8.1f} "
                      f"{traffic / HBM_PEAK * 1e6 / med * 100:6.1f}",
                      flush=True)

            def torch_fwd():
                with torch.no_grad():
                    return Fn.scaled_dot_product_attention(qt, kt, vt)
            row("fwd", lambda: ext.attn_fwd(qkv, h, False), torch_fwd,
                2 * gemm, io)
            row("fwd save", lambda: ext.attn_fwd(qkv, h, True),
                lambda: Fn.scaled_dot_product_attention(qt, kt, vt),
                2 * gemm, io)
            row("bwd", lambda: ext.attn_bwd(qkv, o, lse, do, h),
                lambda: torch.autograd.grad(ot, [qt, kt, vt], dot,
                                            retain_graph=True),
                7 * gemm, 2 * io)
            del qkv, do, qt, kt, vt, dot, ot, o, lse
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn", action="store_true")
    ap.add_argument("--ln", action="store_true")
    ap.add_argument("--blocks", default="",
                    help="further forced grids for --ln's LayerNorm rows, "
                         "comma separated (e.g. 512,4096)")
    ap.add_argument("--se", action="store_true")
    ap.add_argument("--gn", action="store_true")
    ap.add_argument("--gconv", action="store_true")
    ap.add_argument("--dwconv", action="store_true")
    ap.add_argument("--trs", default="",
                    help="further forward strip heights for --dwconv, comma "
                         "separated (e.g. 4,8,32)")
    ap.add_argument("--dwconvk", action="store_true")
    ap.add_argument("--tos", default="",
                    help="further forward run heights for --dwconvk, comma "
                         "separated")
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
    ap.add_argument("--wgradwalk", action="store_true")
    ap.add_argument("--stem", action="store_true")
    ap.add_argument("--linear", action="store_true")
    ap.add_argument("--resnet", action="store_true")
    ap.add_argument("--functional", action="store_true")
    ap.add_argument("--bn", action="store_true")
    ap.add_argument("--bnpool", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if args.attn:
        bench_attn(rounds=30)
        return
    if args.ln:
        bench_ln(rounds=30,
                 blocks=[int(t) for t in args.blocks.split(",") if t])
        return
    if args.se:
        bench_se(rounds=30)
        return
    if args.gn:
        bench_gn(rounds=30)
        return
    if args.gconv:
        bench_gconv(rounds=30)
        return
    if args.dwconvk:
        bench_dwconvk(rounds=30,
                      tos=[int(v) for v in args.tos.split(",") if v])
        return
    if args.dwconv:
        bench_dwconv(rounds=30,
                     trs=[int(v) for v in args.trs.split(",") if v])
        return
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
    if args.wgradwalk:
        bench_wgradwalk(rounds=30)
        return
    if args.stem:
        bench_stem(rounds=30)
        return
    if args.linear:
        bench_linear(rounds=30)
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
