"""SyncBatchNorm entry points in one process: ranks are emulated by sharding
the rows of one tensor, calling bn_sync_local / bn_sync_fwd /
bn_sync_bwd_local / bn_sync_bwd_dx per shard and stacking the local rows
(``torch.stack`` is the gather).  All tests @pytest.mark.gpu.

What is held, and why it must hold (notation, helpers and the float64
bounds are those of test_gpu_norm_exact.py, sections 1 and 2):

* W = 1, any data: the pack kernel repeats k_bn_combine's summation order
  and the cross-rank add starts from row 0, so every output is
  ``torch.equal`` to bn_fwd_train / bn_bwd.
* Any W, sums exact in fp32 (integer / dyadic data, sum|terms| asserted on
  the float64 reference): the order of the additions cannot matter, so the
  concatenated outputs are ``torch.equal`` to the un-sharded kernels.
* Any W, random data: a term passes the additions of its own shard's
  geometry (L_w + T_w as in section 2, for that shard's row count) and then
  at most W rank-order additions, so section 2's bounds hold with
  gamma_s = (max_w (L_w + T_w) + W) * u.  Derived, not measured.
* pre_stats: the conv epilogue sums a 128-row tile per slab entry (a term
  passes at most 128 additions whatever the order inside the tile), then
  the pack's lane sweep and shuffle tree: gamma_pre = (128 + ceil(S/64) + 6)
  * u.  With a 1x1 identity convolution y == x bit for bit, so both rows
  approximate the same float64 sums and differ by at most
  (gamma_pre + gamma_y) * sum|terms|; on integer data both are exact.

Shard counts W in {1, 2, 3, 8} with unequal splits (5 = 4 + 1,
45 = 30 + 14 + 1, ...); a shape appears with every W that leaves each shard
at least one row (one image for the 4-D shape, sharded along N).
"""
import copy
import functools

import pytest
import torch

import test_gpu_norm_exact as nx
from test_gpu_norm_exact import (BF, EPS, EPS32, F64, MOM, R_RSQRT, SLACK, U,
                                 _cdiv, _choice, _dev, _f32, _geom, _ints, _mc,
                                 _pack_mask, _randn, _sid)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

# (shape, what it reaches)
SHAPES = [
    ((5, 8), "M<nw"),
    ((45, 24), "block255"),
    ((300, 2048), "sweep_wraps"),
    ((4, 64, 13, 13), "4d"),
]
WORLDS = [1, 2, 3, 8]


def _units(shape):
    """what is sharded: images for 4-D, rows for 2-D"""
    return shape[0]


def _rows_per_unit(shape):
    return shape[2] * shape[3] if len(shape) == 4 else 1


def _split(n, W):
    """W unequal parts of n, each >= 1: [n], [n-1, 1], [.., .., 1, 1...]"""
    assert n >= W
    if W == 1:
        return [n]
    if W == 2:
        return [n - 1, 1]
    rest = n - (W - 2)
    k = max(1, rest // 3)
    return [rest - k, k] + [1] * (W - 2)


CASES = [(s, W) for s, _ in SHAPES for W in WORLDS if _units(s) >= W]
CASE_IDS = [f"{_sid(s)}-W{W}" for s, W in CASES]


def test_tables_reach_what_they_claim():
    assert _split(5, 2) == [4, 1] and _split(45, 3) == [30, 14, 1]
    for shape, W in CASES:
        parts = _split(_units(shape), W)
        assert len(parts) == W and sum(parts) == _units(shape)
        assert min(parts) >= 1 and (W == 1 or len(set(parts)) > 1)
    for shape, edge in SHAPES:
        M, C = _mc(shape)
        g = _geom(M, C)
        if edge == "M<nw":
            assert M < g["nw"]
        elif edge == "block255":
            assert g["cpg"] == 3 and g["block"] == 255
        elif edge == "sweep_wraps":
            assert g["nw"] == 1 and g["S"] == 75 > 64
        elif edge == "4d":
            assert len(shape) == 4
    # every W occurs, and 8 ranks occur with a wrapped sweep in shard 0
    assert {W for _, W in CASES} == set(WORLDS)
    assert ((300, 2048), 8) in CASES
    assert _geom(_split(300, 8)[0], 2048)["S"] < 64     # shards do not wrap


def _shard(t, shape, W):
    """device tensor of ``shape`` -> list of W views along dim 0"""
    parts = _split(_units(shape), W)
    out, a = [], 0
    for p in parts:
        out.append(t[a:a + p])
        a += p
    return out


def _shard_rows(shape, W):
    return [p * _rows_per_unit(shape) for p in _split(_units(shape), W)]


def _mask_rows(mask, shape, W):
    """[M, C/8] mask -> per-shard row blocks"""
    out, a = [], 0
    for m in _shard_rows(shape, W):
        out.append(mask[a:a + m])
        a += m
    return out


def _sync_fwd(xs, gamma, beta, rm0, rv0, relu, rs):
    """The emulated forward: per rank [y, mean, invstd, mask, count, rm, rv]
    and the stacked rows."""
    rows = [ext.bn_sync_local(x) for x in xs]
    G = torch.stack(rows)
    outs = []
    for w, x in enumerate(xs):
        rm, rv = rm0.clone(), rv0.clone()
        o = ext.bn_sync_fwd(x, G, gamma, beta, rm, rv, MOM, EPS, relu,
                            rs[w] if rs is not None else None)
        assert len(o) == 5
        outs.append(list(o) + [rm, rv])
    return outs, G


def _sync_bwd(xs, dys, gamma, sm, si, masks, relu, count, want_dresid):
    rows = [ext.bn_sync_bwd_local(x, dy, sm, si, m, relu)
            for x, dy, m in zip(xs, dys, masks)]
    G = torch.stack(rows)
    outs = [ext.bn_sync_bwd_dx(x, dy, gamma, sm, si, m, relu, G, count,
                               want_dresid)
            for x, dy, m in zip(xs, dys, masks)]
    return outs, rows


def _assert_ranks_agree(outs, idx, what):
    for o in outs[1:]:
        for i in idx:
            assert torch.equal(o[i], outs[0][i]), (what, i)


def _run_stats(C, key):
    rm0, rv0 = nx._run_stats(C, key)
    return _f32(rm0), _f32(rv0)


# ------------------------------------------- W = 1: bit-identical, any data --

@pytest.mark.parametrize("resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=_sid)
def test_world1_bit_identical_on_random_data(shape, relu, resid):
    M, C = _mc(shape)
    std = 0.5 + _randn((C,), "w1 std").abs()
    x = _dev((_randn((M, C), "w1 x") + 1.0) * std, shape)
    r = _dev(_randn((M, C), "w1 r"), shape) if resid else None
    dy = _dev(_randn((M, C), "w1 dy"), shape)
    gamma = _f32(_randn((C,), "w1 g").double())
    beta = _f32(_randn((C,), "w1 b").double())
    rm0, rv0 = _run_stats(C, "w1")
    rm, rv = rm0.clone(), rv0.clone()
    y, sm, si, mask = ext.bn_fwd_train(x, gamma, beta, rm, rv, MOM, EPS,
                                       relu, r)
    ref_b = ext.bn_bwd(x, dy, gamma, sm, si, mask, relu, resid)
    outs, G = _sync_fwd([x], gamma, beta, rm0, rv0, relu,
                        [r] if resid else None)
    y2, sm2, si2, mask2, count, rm2, rv2 = outs[0]
    assert G.shape == (1, 2 * C + 2) and G.dtype == torch.float32
    assert y2.shape == tuple(shape) and y2.dtype == BF
    if len(shape) == 4:
        assert y2.is_contiguous(memory_format=torch.channels_last)
    assert count.dtype == torch.int64 and count.tolist() == [M]
    for got, ref, name in ((y2, y, "y"), (sm2, sm, "save_mean"),
                           (si2, si, "save_invstd"), (mask2, mask, "mask"),
                           (rm2, rm, "running_mean"), (rv2, rv, "running_var")):
        assert torch.equal(got, ref), name
    assert mask2.shape == ((M, C // 8) if relu else (0,))
    assert not torch.equal(rm2, rm0)            # the blend happened
    bouts, brows = _sync_bwd([x], [dy], gamma, sm2, si2, [mask2], relu,
                             count, resid)
    assert len(bouts[0]) == (2 if resid else 1)
    assert brows[0].shape == (2 * C,)
    assert torch.equal(bouts[0][0], ref_b[0]), "dx"
    assert torch.equal(brows[0][C:], ref_b[1]), "dgamma"
    assert torch.equal(brows[0][:C], ref_b[2]), "dbeta"
    if resid:
        assert torch.equal(bouts[0][1], ref_b[3]), "dresid"


# ------------------------------------------------ any W: forward, exact -----

@functools.lru_cache(maxsize=None)
def _fwd_case(shape):
    """Integer inputs, the float64 exactness precondition, and the
    un-sharded bn_fwd_train outputs (computed once per shape, read-only)."""
    M, C = _mc(shape)
    x = _ints((M, C), -4, 4, "sync fwd x")
    r = _ints((M, C), -3, 3, "sync fwd r")
    assert x.abs().sum(0).max().item() < 2 ** 24
    assert (x * x).sum(0).max().item() < 2 ** 24
    gamma = _f32(_choice([0.5, 1.0, 2.0], C, "sync fwd g"))
    beta = _f32(_choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, "sync fwd b"))
    rm0, rv0 = _run_stats(C, "sync fwd")
    xd, rd = _dev(x, shape), _dev(r, shape)
    ref = {}
    for relu in (False, True):
        for resid in (False, True):
            rm, rv = rm0.clone(), rv0.clone()
            o = ext.bn_fwd_train(xd, gamma, beta, rm, rv, MOM, EPS, relu,
                                 rd if resid else None)
            ref[relu, resid] = list(o) + [rm, rv]
    return x, xd, rd, gamma, beta, rm0, rv0, ref


@pytest.mark.parametrize("shape,W", CASES, ids=CASE_IDS)
def test_forward_exact_any_world(shape, W):
    M, C = _mc(shape)
    x, xd, rd, gamma, beta, rm0, rv0, ref = _fwd_case(shape)
    xs, rs = _shard(xd, shape, W), _shard(rd, shape, W)
    ms = _shard_rows(shape, W)
    for relu, resid in ((False, False), (True, True), (True, False)):
        outs, G = _sync_fwd(xs, gamma, beta, rm0, rv0, relu,
                            rs if resid else None)
        what = f"{shape} W={W} relu={relu} resid={resid}"
        # the rows: exact local sums, and the count in two exact slots
        a = 0
        for w, m in enumerate(ms):
            xw = x[a:a + m]
            a += m
            g = G[w].cpu().double()
            assert torch.equal(g[:C], xw.sum(0)), what
            assert torch.equal(g[C:2 * C], (xw * xw).sum(0)), what
            assert g[2 * C:].tolist() == [m >> 12, m & 4095], what
        _assert_ranks_agree(outs, (1, 2, 4, 5, 6), what)
        y, sm, si, mask, rm, rv = ref[relu, resid]
        o = outs[0]
        assert o[4].tolist() == [M], what
        assert torch.equal(o[1], sm) and torch.equal(o[2], si), what
        assert torch.equal(o[5], rm) and torch.equal(o[6], rv), what
        assert torch.equal(torch.cat([o[0] for o in outs]), y), what
        if relu:
            assert torch.equal(torch.cat([o[3] for o in outs]), mask), what
        else:
            assert all(o[3].numel() == 0 for o in outs)


def test_count_slots_past_2_pow_24():
    """A local row count that no single fp32 holds: 2^24 + 1 rows of 8
    channels (256 MiB of bf16), two emulated ranks of that and 5 rows."""
    C = 8
    M0 = 2 ** 24 + 1
    x0 = torch.ones(M0, C, dtype=BF, device=DEV)
    x1 = torch.ones(5, C, dtype=BF, device=DEV)
    rows = [ext.bn_sync_local(x0), ext.bn_sync_local(x1)]
    assert rows[0][2 * C:].tolist() == [M0 >> 12, M0 & 4095] == [4096, 1]
    G = torch.stack(rows)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    o = ext.bn_sync_fwd(x1, G, torch.ones(C, device=DEV),
                        torch.zeros(C, device=DEV), rm, rv, MOM, EPS, False)
    assert o[4].tolist() == [M0 + 5]
    # sum = 2^24 + 6 is exact in the slab (each split holds far fewer than
    # 2^24 ones); the last adds, the conversion of M and the division round
    # once each: mean = 1 within 4u
    assert abs(float(o[1][0]) - 1.0) <= 4 * U


# ----------------------------------------------- any W: backward, exact -----

@functools.lru_cache(maxsize=None)
def _bwd_case(shape):
    """test_gpu_norm_exact's dyadic recipe and the un-sharded bn_bwd."""
    M, C = _mc(shape)
    x, dy, mean, invstd, gamma, bits = nx._bwd_case(M, C)
    xhat = (x - mean) * invstd
    ref = {}
    for relu in (False, True):
        dy_eff = dy * bits if relu else dy
        assert dy_eff.abs().sum(0).max().item() < 2 ** 23
        assert (dy_eff * xhat).abs().sum(0).max().item() < 2 ** 23
        mask = _pack_mask(bits).to(DEV) if relu \
            else torch.empty(0, dtype=torch.uint8, device=DEV)
        out = ext.bn_bwd(_dev(x, shape), _dev(dy, shape), _f32(gamma),
                         _f32(mean), _f32(invstd), mask, relu, relu)
        ref[relu] = (mask, out, dy_eff.sum(0), (dy_eff * xhat).sum(0))
    return x, dy, mean, invstd, gamma, ref


@pytest.mark.parametrize("shape,W", CASES, ids=CASE_IDS)
def test_backward_exact_any_world(shape, W):
    M, C = _mc(shape)
    x, dy, mean, invstd, gamma, ref = _bwd_case(shape)
    xs = _shard(_dev(x, shape), shape, W)
    dys = _shard(_dev(dy, shape), shape, W)
    count = torch.tensor([M], dtype=torch.int64, device=DEV)
    for relu in (False, True):
        mask, out, dbeta64, dgamma64 = ref[relu]
        masks = _mask_rows(mask, shape, W) if relu else [mask] * W
        bouts, brows = _sync_bwd(xs, dys, _f32(gamma), _f32(mean),
                                 _f32(invstd), masks, relu, count, relu)
        what = f"{shape} W={W} relu={relu}"
        assert torch.equal(torch.cat([o[0] for o in bouts]), out[0]), what
        if relu:
            assert torch.equal(torch.cat([o[1] for o in bouts]), out[3]), what
        loc = torch.stack(brows).cpu().double().sum(0)
        assert torch.equal(loc[:C], dbeta64), what
        assert torch.equal(loc[C:], dgamma64), what
        assert torch.equal(loc[:C], out[2].cpu().double()), what
        assert torch.equal(loc[C:], out[1].cpu().double()), what


# ------------------------------------------------- any W: random tier -------

def _stat_bounds_gamma(x, gam):
    """test_gpu_norm_exact._stat_bounds(x, False) with gamma_s handed in."""
    M, C = x.shape
    a1, s2 = x.abs().sum(0), (x * x).sum(0)
    mean, msq = x.sum(0) / M, s2 / M
    var = (msq - mean * mean).clamp_min(0)
    e_mean = gam * a1 / M + U * mean.abs()
    e_msq = gam * msq + U * msq
    e_var = (e_msq + 2 * mean.abs() * e_mean + e_mean ** 2
             + 3 * U * (msq + mean * mean)) * SLACK
    lo_a = (var + EPS32 - e_var) * (1 - U)
    hi_a = (var + EPS32 + e_var) * (1 + U)
    assert lo_a.min().item() > 0
    inv = (var + EPS32) ** -0.5
    inv_lo = hi_a ** -0.5 * (1 - 2 * R_RSQRT * U * SLACK)
    inv_hi = lo_a ** -0.5 * (1 + 2 * R_RSQRT * U * SLACK)
    assert M > 1
    unb = var * M / (M - 1)
    e_unb = (e_var * M / (M - 1) + 2 * U * unb) * SLACK
    return dict(mean=mean, var=var, e_mean=e_mean, e_var=e_var, inv=inv,
                inv_lo=inv_lo, inv_hi=inv_hi, unb=unb, e_unb=e_unb,
                gamma_s=gam)


def _additions(shape, W):
    C = _mc(shape)[1]
    geoms = [_geom(m, C) for m in _shard_rows(shape, W)]
    return max(g["L"] + g["T"] for g in geoms) + W


def test_random_tier_bound_matches_the_unsharded_one_at_world1():
    for shape, _ in SHAPES:
        M, C = _mc(shape)
        x = _randn((M, C), "bound check").to(BF).double()
        a = _stat_bounds_gamma(x, (_additions(shape, 1) - 1) * U)
        b = nx._stat_bounds(x, False)
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k


@pytest.mark.parametrize("ratio", [0, 4])
@pytest.mark.parametrize("shape,W", CASES, ids=CASE_IDS)
def test_forward_stats_random_any_world(shape, W, ratio):
    M, C = _mc(shape)
    std = 0.5 + _randn((C,), "std").abs()
    x = ((_randn((M, C), "rand x") + float(ratio)) * std).to(BF).double()
    T = _additions(shape, W)
    assert T < 5792
    st = _stat_bounds_gamma(x, T * U)
    rm0, rv0 = _run_stats(C, "sync rand")
    xs = _shard(_dev(x, shape), shape, W)
    outs, _ = _sync_fwd(xs, _f32(torch.ones(C)), _f32(torch.zeros(C)), rm0,
                        rv0, False, None)
    what = f"sync rand {shape} W={W} mean/std={ratio}"
    _assert_ranks_agree(outs, (1, 2, 4, 5, 6), what)
    o = outs[0]
    assert o[4].tolist() == [M]
    nx._check_stats(st, o[1], o[2], o[5], o[6], rm0.cpu().double(),
                    rv0.cpu().double(), what)


# ------------------------------------------------------------ pre_stats -----

def _act(t64):
    return t64.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) \
        .to(DEV)


# N, C, H, W, K, R, S, stride, pad: one tile, and two tiles with a row over
PRE_INT_SHAPES = [(2, 8, 5, 7, 8, 3, 3, 1, 1), (1, 8, 3, 43, 64, 1, 1, 1, 0)]


@pytest.mark.parametrize("shape", PRE_INT_SHAPES, ids=_sid)
def test_pre_stats_row_exact_on_integer_data(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    x = _ints((N, C, H, W), -2, 2, "pre x")
    w = _ints((K, C, R, S), -1, 1, "pre w")
    b = _ints((K,), -3, 3, "pre b")
    v = torch.nn.functional.conv2d(x, w, b, stride, pad)
    absv = torch.nn.functional.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
    assert absv.max().item() <= 256          # y is exact in bf16
    assert (v * v).sum((0, 2, 3)).max().item() < 2 ** 24
    y, slab = ext.conv2d_fwd_stats(_act(x), _act(w), b.float().to(DEV),
                                   stride, pad)
    M = N * v.shape[2] * v.shape[3]
    assert slab.shape == (2, K, _cdiv(M, 128))
    row_pre = ext.bn_sync_local(y, slab)
    row_y = ext.bn_sync_local(y)
    assert torch.equal(row_pre, row_y)
    g = row_pre.cpu().double()
    assert torch.equal(g[:K], v.sum((0, 2, 3)))
    assert torch.equal(g[K:2 * K], (v * v).sum((0, 2, 3)))
    assert g[2 * K:].tolist() == [0, M]


def test_pre_stats_row_within_the_band_on_random_data():
    """1x1 identity convolution: y == x bit for bit, random bf16 data at
    mean/std = 4, four 128-row tiles with a partial last one."""
    N, C, H, W = 3, 64, 13, 13
    M = N * H * W
    std = 0.5 + _randn((C,), "pre std").abs()
    xr = ((_randn((M, C), "pre rand x") + 4.0) * std).to(BF).double()
    xd = _dev(xr, (N, C, H, W))
    w = torch.eye(C, dtype=F64).view(C, C, 1, 1)
    y, slab = ext.conv2d_fwd_stats(xd, _act(w), None, 1, 0)
    assert torch.equal(y, xd)
    S = _cdiv(M, 128)
    assert slab.shape == (2, C, S) and S == 4 and M % 128
    row_pre = ext.bn_sync_local(y, slab).cpu().double()
    row_y = ext.bn_sync_local(y).cpu().double()
    assert torch.equal(row_pre[2 * C:], row_y[2 * C:])
    assert row_y[2 * C:].tolist() == [0, M]
    g = _geom(M, C)
    gam_y = (g["L"] + g["T"]) * U
    gam_pre = (128 + _cdiv(S, 64) + 6) * U
    a1, s2 = xr.abs().sum(0), (xr * xr).sum(0)
    for name, lo, truth, mag in (("sum", 0, xr.sum(0), a1),
                                 ("sumsq", C, s2, s2)):
        p, q = row_pre[lo:lo + C], row_y[lo:lo + C]
        nx._assert_within(q, truth, gam_y * mag * SLACK, f"row_y {name}")
        nx._assert_within(p, truth, gam_pre * mag * SLACK, f"row_pre {name}")
        nx._assert_within(p, q, (gam_pre + gam_y) * mag * SLACK,
                          f"row_pre vs row_y {name}")


# --------------------------------------------- module level, no group -------

def test_converted_block_is_bit_identical_without_a_process_group():
    import torch.distributed as dist

    from ddp_tricks_amd.models.resnet import BasicBlock
    from ddp_tricks_amd.ops.modules import SyncBatchNorm
    from ddp_tricks_amd.parallel import convert_sync_batchnorm
    # (an earlier test of the session may have left a one-rank group)
    assert not dist.is_initialized() or dist.get_world_size() == 1
    torch.manual_seed(5)
    plain = BasicBlock(16, 16).to(DEV)
    with torch.no_grad():
        for bn in (plain.bn1, plain.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_()
    sync = convert_sync_batchnorm(copy.deepcopy(plain))
    assert isinstance(sync.bn1, SyncBatchNorm) and sync.bn1.fuse_relu
    assert isinstance(sync.bn2, SyncBatchNorm)
    assert list(sync.state_dict().keys()) == list(plain.state_dict().keys())
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(3, 16, 9, 7, generator=g).to(BF).to(DEV) \
        .contiguous(memory_format=torch.channels_last)
    dy = torch.randn(3, 16, 9, 7, generator=g).to(BF).to(DEV) \
        .contiguous(memory_format=torch.channels_last)
    res = []
    for model in (plain, sync):
        model.train()
        x = x0.clone().requires_grad_(True)
        y = model(x)
        y.backward(dy)
        res.append((y.detach(), x.grad,
                    {k: p.grad for k, p in model.named_parameters()},
                    {k: b for k, b in model.named_buffers()}))
    (y0, dx0, g0, b0), (y1, dx1, g1, b1) = res
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    for k in b0:
        assert torch.equal(b1[k], b0[k]), k
    assert int(b1["bn1.num_batches_tracked"]) == 1


def test_entry_points_refuse_what_they_cannot_index():
    C = 16
    x = torch.zeros(4, C, dtype=BF, device=DEV)
    f = torch.zeros(C, device=DEV)
    with pytest.raises(RuntimeError):
        ext.bn_sync_local(torch.zeros(4, 12, dtype=BF, device=DEV))
    with pytest.raises(RuntimeError):       # pre_stats of another C
        ext.bn_sync_local(x, torch.zeros(2, 8, 1, device=DEV))
    with pytest.raises(RuntimeError):       # rows of the backward's width
        ext.bn_sync_fwd(x, torch.zeros(2, 2 * C, device=DEV), f, f, f, f,
                        MOM, EPS, False)
    with pytest.raises(RuntimeError):       # rows of the forward's width
        ext.bn_sync_bwd_dx(x, x, f, f, f, torch.empty(0, dtype=torch.uint8,
                                                       device=DEV), False,
                           torch.zeros(2, 2 * C + 2, device=DEV),
                           torch.ones(1, dtype=torch.int64, device=DEV),
                           False)
    with pytest.raises(RuntimeError):       # relu without its mask
        ext.bn_sync_bwd_local(x, x, f, f, torch.empty(0, dtype=torch.uint8,
                                                      device=DEV), True)


# ------------------------------------------------- rccl_all_gather, W = 1 ---

@pytest.mark.timeout(300)
def test_rccl_all_gather_world1_is_the_identity():
    """test_rccl_world1_collectives' pattern: a real communicator of one
    rank, the collective enqueued on a side stream behind an event."""
    assert hasattr(ext, "rccl_all_gather")
    comm = ext.rccl_comm_init(1, 0, ext.rccl_unique_id())
    torch.cuda.set_device(0)
    side = torch.cuda.Stream(device=DEV)
    row = torch.arange(34, dtype=torch.float32, device=DEV)
    row.mul_(0.5)
    out = torch.full((1, 34), -1.0, device=DEV)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(DEV))
    side.wait_event(ev)
    with torch.cuda.stream(side):
        ext.rccl_all_gather(row, out, comm)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out[0], torch.arange(34, device=DEV) * 0.5)
    with pytest.raises(RuntimeError):       # dst of the wrong size
        ext.rccl_all_gather(row, torch.empty(2, 34, device=DEV), comm)
    ext.rccl_comm_destroy(comm)
