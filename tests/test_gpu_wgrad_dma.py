"""k_conv_wgrad_wide_dma: the LDS-DMA staged, transposed-read wide wgrad leaf.

The leaf is chosen by DDPX_WGRAD_V, which the extension reads once per
process, so every leaf's outputs come from a child process of its own (this
file run as a script) that writes them to a temporary directory: ``wt`` is
the new leaf at the host's automatic depth, ``wp`` / ``wq`` are the 64- and
32-deep wide_pair leaves it is compared with.  The three children run side
by side, once per session; the tests only compare what they saved.  The new
leaf is forced whatever the automatic dispatch routes to it.

Method of test_gpu_exact.py / test_gpu_wgrad_bias.py, all @pytest.mark.gpu:

* exact: dy, x integers in {-2..2} held in bf16, float64 CPU reference
  (``torch.nn.grad.conv2d_weight``, ``dy.sum((0, 2, 3))``).  The sum of
  |terms| is at most 4*M <= 67 584 < 2^24 (asserted on the reference alone),
  so fp32 accumulation is exact in any order: ``torch.equal`` on dw and db,
  with and without bias.
* random bf16 data: dw must be bit-equal to the wide_pair leaf of the same
  depth (same split, zero fills and MFMA order); db is held element-wise to
  |err| <= gamma * sum|dy| against float64 with ``_wide_pair_gamma`` as in
  test_gpu_wgrad_bias.py (the new leaf keeps the chain that bound assumes:
  two accumulators per ko, DEPTH/2 rows of each tile each, joined once);
  two calls give equal bits.

``_wide_pair_gamma`` is copied except for its "reaches wide_pair" assertion:
a forced ``w*`` letter needs only Ko >= 128 and Kgemm >= 128, and the
(5,128,7,6,128,3,1,1,0) case has 3 tiles.  For the 32-deep class the host's
split loop counts with depth 64, so it stops one doubling earlier than the
copied loop and the copied gamma is SMALLER than the rigorous one (158u
against 282u at M = 16896): the check asks more, not less.
"""
import functools
import os
import subprocess
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)
U = 2.0 ** -24

# (N, C, H, W, K, R, S, stride, pad)
SHAPES = [
    (2, 128, 5, 6, 128, 3, 3, 1, 1),     # DEPTH 64, M = 60 < DEPTH: zero m
                                         # tail in the only tile, padding taps
    (2, 136, 5, 6, 136, 3, 3, 1, 1),     # Ko and Kgemm tails of the 128 tiles
    (2, 56, 6, 5, 136, 3, 3, 1, 1),      # DEPTH 32, Kgemm = 504: tiles
                                         # straddle taps
    (3, 128, 9, 7, 128, 3, 3, 2, 1),     # stride 2, H != W
    (5, 128, 7, 6, 128, 3, 1, 1, 0),     # R != S, pad 0, M = 150
    (16, 56, 33, 32, 136, 3, 3, 1, 1),   # M = 16896: S > 16, two-stage
                                         # combine, several tiles per split
]
KINDS = ("int", "rand")
LEAVES = ("wt", "wp", "wq")
SMALLEST = (2, 8, 5, 7, 8, 3, 3, 1, 1)   # for the unknown-override child


# ---------------------------------------------------------------- helpers ---

def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(shape, lo, hi, *key):
    g = torch.Generator().manual_seed(_seed(shape, lo, hi, *key))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _randn_bf16(shape, *key):
    """float64 CPU tensor of bf16-representable normal values."""
    g = torch.Generator().manual_seed(_seed(shape, *key))
    return torch.randn(tuple(shape), generator=g).to(BF).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _cdiv(a, b):
    return -(-a // b)


def _m_kgemm(shape):
    N, C, H, W, K, R, S, stride, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    return N * P * Q, R * S * C


def _depth(shape):
    return 64 if _m_kgemm(shape)[1] >= 1152 else 32


def _old_leaf(shape):
    return "wp" if _depth(shape) == 64 else "wq"


def _wide_pair_gamma(M, Ko, Kgemm):
    assert Ko >= 128 and Kgemm >= 128
    depth = 64 if Kgemm >= 1152 else 32
    tiles = _cdiv(Ko, 128) * _cdiv(Kgemm, 128)
    S = 1
    while tiles * S < 1024 and S < 512 and M // (S * 2 * depth) >= 8:
        S *= 2
    L = _cdiv(_cdiv(M, depth), S) * (depth // 2) + 1
    T = S if S <= 16 else 4 + 1 + _cdiv(S, 8)
    return (L + T) * U, S


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """(x, dy) as float64 CPU tensors; same values in every process."""
    N, C, H, W, K, R, S, stride, pad = shape
    P, Q = _out_hw(H, W, R, S, stride, pad)
    if kind == "int":
        return (_ints((N, C, H, W), -2, 2, "x"),
                _ints((N, K, P, Q), -2, 2, "dy"))
    return _randn_bf16((N, C, H, W), "x"), _randn_bf16((N, K, P, Q), "dy")


@functools.lru_cache(maxsize=None)
def _refs(shape, kind):
    """float64 references, computed once and shared read-only:
    (dw_ref, dw_abs, db_ref, db_abs)."""
    N, C, H, W, K, R, S, stride, pad = shape
    x, dy = _inputs(shape, kind)
    dw = torch.nn.grad.conv2d_weight(x, (K, C, R, S), dy, stride=stride,
                                     padding=pad)
    dw_abs = torch.nn.grad.conv2d_weight(x.abs(), (K, C, R, S), dy.abs(),
                                         stride=stride, padding=pad)
    return dw, dw_abs, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


# ------------------------------------------------------------------ child ---

def _child(out_path):
    """Runs every case this process's DDPX_WGRAD_V leaf is needed for and
    saves {(shape, kind): (dw_plain, dw, db, dw2, db2)} as CPU tensors, and
    {("plan", shape): conv2d_wgrad_plan's (leaf name, split, fused_bias)}.
    A value that names no leaf (test_unknown_override_is_an_error) gets one
    conv2d_wgrad call on SMALLEST, which must raise."""
    sys.path.insert(0, REPO)
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    dev = torch.device("cuda:0")
    leaf = os.environ["DDPX_WGRAD_V"]
    if leaf not in LEAVES:
        N, C, H, W, K, R, S, stride, pad = SMALLEST
        x, dy = _inputs(SMALLEST, "int")
        ext.conv2d_wgrad(_nhwc(dy.to(BF)).to(dev), _nhwc(x.to(BF)).to(dev),
                         R, S, stride, pad)
        torch.cuda.synchronize()
        return
    out = {}
    for shape in SHAPES:
        if leaf != "wt" and leaf != _old_leaf(shape):
            continue
        N, C, H, W, K, R, S, stride, pad = shape
        out[("plan", shape)] = ext.conv2d_wgrad_plan(*shape, True)
        for kind in KINDS:
            if leaf != "wt" and kind == "int":
                continue
            x, dy = _inputs(shape, kind)
            xd = _nhwc(x.to(BF)).to(dev)
            dyd = _nhwc(dy.to(BF)).to(dev)
            dw_plain = ext.conv2d_wgrad(dyd, xd, R, S, stride, pad)
            dw, db = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
            dw2, db2 = ext.conv2d_wgrad_bias(dyd, xd, R, S, stride, pad)
            out[(shape, kind)] = tuple(
                t.cpu() for t in (dw_plain, dw, db, dw2, db2))
    torch.cuda.synchronize()
    torch.save(out, out_path)


@pytest.fixture(scope="module")
def leaf_out(tmp_path_factory):
    """{leaf letter: child's saved dict}; one fresh process per leaf."""
    d = tmp_path_factory.mktemp("wgrad_dma")
    procs = {}
    for leaf in LEAVES:
        env = dict(os.environ)
        env["DDPX_WGRAD_V"] = leaf
        procs[leaf] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--child",
             str(d / f"{leaf}.pt")],
            cwd=REPO, env=env, stdout=subprocess.PIPE,
            stderr=subprocess.PIPE, text=True)
    res = {}
    for leaf, p in procs.items():
        try:
            _, err = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, (leaf, err[-2000:])
        res[leaf] = torch.load(str(d / f"{leaf}.pt"), weights_only=False)
    return res


# ------------------------------------------------------------------ tests ---

def test_shapes_reach_what_they_claim():
    for shape in SHAPES:
        M, Kgemm = _m_kgemm(shape)
        assert shape[4] >= 128 and Kgemm >= 128     # a forced w* letter
        assert 4 * M <= 67584
    assert _depth(SHAPES[0]) == 64 and _m_kgemm(SHAPES[0])[0] < 64
    assert SHAPES[1][4] % 128 and _m_kgemm(SHAPES[1])[1] % 128
    assert _depth(SHAPES[2]) == 32 and _m_kgemm(SHAPES[2])[1] == 504
    assert _m_kgemm(SHAPES[4])[0] == 150
    M, Kgemm = _m_kgemm(SHAPES[5])
    # the host's split loop counts with depth 64 on every wide leaf
    S = 1
    while 8 * S < 1024 and S < 512 and M // (S * 128) >= 8:
        S *= 2
    assert M == 16896 and S > 16 and _cdiv(_cdiv(M, 32), S) > 1


def test_children_ran_the_leaf_they_were_forced_to(leaf_out):
    """What the host's own plan reported in each child."""
    for shape in SHAPES:
        depth = _depth(shape)
        new, old = leaf_out["wt"], leaf_out[_old_leaf(shape)]
        assert new[("plan", shape)][0] == f"wide_dma<{depth}>"
        assert old[("plan", shape)][0] == f"wide_pair<{depth}>"
        # same split and both with the bias fused: dw is comparable bit by bit
        assert new[("plan", shape)][1:] == old[("plan", shape)][1:]
        assert new[("plan", shape)][2] is True
    # the split test_shapes_reach_what_they_claim works out for the last shape
    M, _ = _m_kgemm(SHAPES[5])
    S = 1
    while 8 * S < 1024 and S < 512 and M // (S * 128) >= 8:
        S *= 2
    assert leaf_out["wt"][("plan", SHAPES[5])][1] == S


def test_unknown_override_is_an_error(tmp_path):
    """A DDPX_WGRAD_V value that names no leaf must stop the first wgrad call
    with the accepted spellings, not run some other kernel silently."""
    env = dict(os.environ)
    env["DDPX_WGRAD_V"] = "zz"
    p = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--child",
         str(tmp_path / "zz.pt")],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode != 0, p.stderr[-2000:]
    assert "DDPX_WGRAD_V=zz" in p.stderr, p.stderr[-2000:]
    assert "wt, wt3, wp, wq, s, sb, s6" in p.stderr, p.stderr[-2000:]


@pytest.mark.parametrize("shape", SHAPES)
def test_dma_exact(shape, leaf_out):
    N, C, H, W, K, R, S, stride, pad = shape
    dw_ref, dw_abs, db_ref, db_abs = _refs(shape, "int")
    assert dw_abs.max().item() < EXACT_LIMIT
    assert db_abs.max().item() < EXACT_LIMIT
    dw_plain, dw, db, _, _ = leaf_out["wt"][(shape, "int")]
    assert dw.dtype == torch.float32 and dw.shape == (K, C, R, S)
    assert db.dtype == torch.float32 and db.shape == (K,)
    assert torch.equal(dw_plain.double(), dw_ref)
    assert torch.equal(dw.double(), dw_ref)
    assert torch.equal(db.double(), db_ref)


def _assert_within(got, ref, abs_sum, gamma, what):
    err = (got.double() - ref).abs()
    bound = gamma * abs_sum
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}, gamma {gamma:.3e}")
    assert worst <= 0.0, (what, worst)


@pytest.mark.parametrize("shape", SHAPES)
def test_dma_random(shape, leaf_out):
    K = shape[4]
    _, _, db_ref, db_abs = _refs(shape, "rand")
    M, Kgemm = _m_kgemm(shape)
    gamma, _ = _wide_pair_gamma(M, K, Kgemm)
    dw_plain, dw, db, dw2, db2 = leaf_out["wt"][(shape, "rand")]
    old_plain, old_dw, _, _, _ = leaf_out[_old_leaf(shape)][(shape, "rand")]
    assert torch.equal(dw_plain, old_plain)
    assert torch.equal(dw, old_dw)
    assert torch.equal(dw, dw_plain)
    _assert_within(db, db_ref, db_abs, gamma, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
