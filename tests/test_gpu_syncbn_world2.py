"""SyncBatchNorm across two real ranks on ONE device: two spawned processes,
both on cuda:0, torch process group on gloo (tests/test_gpu_rccl.py's rig),
so the gather is the zero-padded all-reduce of device tensors.

Each rank runs ``SyncBatchNorm(fuse_relu=True)`` with a residual on its
share (3 + 1 images) of a seeded integer batch, through autograd.  Integer
x in {-4..4} keeps the sums exact in fp32, so the order of the cross-rank
additions cannot matter and the full-batch ``BatchNorm2d`` of the parent
process is a bit-exact reference for y and the statistics.  dx and the
parameter gradients are compared with the single-process emulation of
test_gpu_syncbn.py (the four entry points per shard, ``torch.stack`` as the
gather): the transport changes the bytes moved, not the arithmetic.

At most three processes hold the GPU; nothing is retried.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

WORLD = 2
SHAPE = (4, 16, 6, 5)
SPLIT = (3, 1)
MOM, EPS = 0.1, 1e-5
BF = torch.bfloat16


def _case():
    g = torch.Generator().manual_seed(2024)
    N, C, H, W = SHAPE

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def cl(t):
        return t.to(BF).contiguous(memory_format=torch.channels_last)
    x = cl(ints(-4, 4, *SHAPE))
    r = cl(ints(-3, 3, *SHAPE))
    dy = cl(ints(-2, 2, *SHAPE))
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,),
                                                        generator=g)]
    beta = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (C,),
                                                              generator=g)]
    rm0 = torch.randn(C, generator=g)
    rv0 = torch.rand(C, generator=g) + 0.5
    return x, r, dy, gamma, beta, rm0, rv0


def _load(bn, gamma, beta, rm0, rv0):
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)


def _np(t):
    return t.detach().float().cpu().numpy()


def _worker(rank, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)            # BOTH ranks share device 0
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from ddp_tricks_amd.ops.modules import SyncBatchNorm
    x, r, dy, gamma, beta, rm0, rv0 = _case()
    lo = sum(SPLIT[:rank])
    hi = lo + SPLIT[rank]
    bn = SyncBatchNorm(SHAPE[1], fuse_relu=True).cuda()
    _load(bn, gamma, beta, rm0, rv0)
    bn.train()
    xs = x[lo:hi].cuda().requires_grad_(True)
    rs = r[lo:hi].cuda().requires_grad_(True)
    y = bn(xs, residual=rs)
    _, _, save_mean, save_invstd, _, count = y.grad_fn.saved_tensors
    y.backward(dy[lo:hi].cuda())
    torch.cuda.synchronize()
    results.put((rank, dict(
        y=_np(y), dx=_np(xs.grad), dr=_np(rs.grad), gw=_np(bn.weight.grad),
        gb=_np(bn.bias.grad), sm=_np(save_mean), si=_np(save_invstd),
        rm=_np(bn.running_mean), rv=_np(bn.running_var),
        count=int(count.item()), nbt=int(bn.num_batches_tracked))))
    dist.barrier()
    dist.destroy_process_group()


def _eq(a, t):
    return torch.equal(torch.from_numpy(a), t.detach().float().cpu())


@pytest.mark.timeout(600)
def test_world2_sync_batchnorm_matches_full_batch_and_emulation():
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 29731, results))
             for r in range(WORLD)]
    [p.start() for p in procs]
    got = dict(results.get(timeout=240) for _ in range(WORLD))
    [p.join(timeout=120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)

    from ddp_tricks_amd.ops import load_extension
    from ddp_tricks_amd.ops.modules import BatchNorm2d
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    x, r, dy, gamma, beta, rm0, rv0 = _case()
    N, C, H, W = SHAPE
    M = N * H * W
    # the sums are exact in fp32 in any order
    assert x.double().abs().sum((0, 2, 3)).max().item() < 2 ** 24
    assert (x.double() ** 2).sum((0, 2, 3)).max().item() < 2 ** 24

    # both ranks hold the same statistics, bit for bit
    for k in ("sm", "si", "rm", "rv"):
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    assert got[0]["count"] == got[1]["count"] == M
    assert got[0]["nbt"] == got[1]["nbt"] == 1

    # forward: the parent's full-batch BatchNorm2d
    full = BatchNorm2d(C, fuse_relu=True).to(dev)
    _load(full, gamma.to(dev), beta.to(dev), rm0.to(dev), rv0.to(dev))
    full.train()
    xf = x.to(dev).requires_grad_(True)
    yf = full(xf, residual=r.to(dev))
    _, _, sm_f, si_f, mask_f = yf.grad_fn.saved_tensors
    bounds = [(sum(SPLIT[:k]), sum(SPLIT[:k + 1])) for k in range(WORLD)]
    for rank, (lo, hi) in enumerate(bounds):
        assert _eq(got[rank]["y"], yf[lo:hi]), rank
        assert _eq(got[rank]["sm"], sm_f) and _eq(got[rank]["si"], si_f)
        assert _eq(got[rank]["rm"], full.running_mean), rank
        assert _eq(got[rank]["rv"], full.running_var), rank

    # backward: the single-process emulation, shard by shard
    xd, dyd = x.to(dev), dy.to(dev)
    xs = [xd[lo:hi] for lo, hi in bounds]
    dys = [dyd[lo:hi] for lo, hi in bounds]
    masks = [mask_f[lo * H * W:hi * H * W] for lo, hi in bounds]
    rows = [ext.bn_sync_bwd_local(a, b, sm_f, si_f, m, True)
            for a, b, m in zip(xs, dys, masks)]
    G = torch.stack(rows)
    count = torch.tensor([M], dtype=torch.int64, device=dev)
    g32 = gamma.to(dev)
    for rank in range(WORLD):
        dx, dresid = ext.bn_sync_bwd_dx(xs[rank], dys[rank], g32, sm_f, si_f,
                                        masks[rank], True, G, count, True)
        assert _eq(got[rank]["dx"], dx), rank
        assert _eq(got[rank]["dr"], dresid), rank
        assert _eq(got[rank]["gb"], rows[rank][:C]), rank
        assert _eq(got[rank]["gw"], rows[rank][C:]), rank
    # the gradients are not all zero (the relu mask lets something through)
    assert any(got[k]["dx"].any() for k in range(WORLD))
    assert got[0]["gw"].any() and got[0]["gb"].any()
