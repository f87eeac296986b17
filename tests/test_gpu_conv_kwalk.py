"""Scalar tap walk of the conv GEMM K loop (`kwalk` argument of
`conv2d_fwd`, `conv2d_fwd_stats` and `conv2d_dgrad`, `conv2d_kloop_plan`;
docs/KERNELS.md "K loop: scalar tap walk").

With kwalk = 1 the K loop carries (r, s, channel base) as scalars and forms
every source address from a cached per-lane offset; with kwalk = 0 it decodes
(r, s, c) per chunk.  Both stage the same LDS images in the same K-tile order
and run the same MFMAs, so every case compares kwalk = 1 against kwalk = 0 by
``torch.equal`` on random bf16 data, and asserts that ``conv2d_kloop_plan``
names the path that ran: "walk" where the contraction channels (C forward,
Ko stride-1 dgrad) are a multiple of 64, "decode" otherwise and under
kwalk = 0.  The references of both paths are pinned by test_gpu_exact.py,
test_gpu_autograd_exact.py and test_gpu_dgrad_taps.py, which run the
automatic path.

Geometries keep N*P*Q off the 128-row tile: below one tile, and above one
but no multiple of it.  All tests @pytest.mark.gpu.
"""
import itertools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

BF = torch.bfloat16
CL = torch.channels_last

# (N, H, W): N*P*Q < 128 for every filter below, and > 128 but no multiple
GEOS = [(2, 6, 7), (3, 9, 8)]
FWD_C = [64, 128, 192]
FWD_KO = [64, 128, 136]
FILTERS = [(1, 1), (3, 3), (3, 1), (1, 3), (5, 5)]


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(
        zlib.crc32(repr(key).encode()))


def _act(shape, g):
    return torch.randn(shape, device=DEV, generator=g).to(BF) \
        .contiguous(memory_format=CL)


def _fwd_pair(N, C, H, W, Ko, R, S, stride, pad, stats, bias):
    """y (and the stats slab) under kwalk = 1 and kwalk = 0."""
    g = _gen("fwd", N, C, H, W, Ko, R, S, stride, pad)
    x = _act((N, C, H, W), g)
    w = _act((Ko, C, R, S), g)
    b = torch.randn(Ko, device=DEV, generator=g) if bias else None
    out = []
    for kwalk in (1, 0):
        if stats:
            y, slab = ext.conv2d_fwd_stats(x, w, b, stride, pad, kwalk)
            out.append((y, slab))
        else:
            out.append((ext.conv2d_fwd(x, w, b, stride, pad, kwalk),))
    return out


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("R,S", FILTERS)
@pytest.mark.parametrize("Ko", FWD_KO)
@pytest.mark.parametrize("C", FWD_C)
def test_forward_walk_equals_decode(C, Ko, R, S, pad, stride):
    tiles = set()
    for (N, H, W), stats in itertools.product(GEOS, (False, True)):
        if H + 2 * pad < R or W + 2 * pad < S:
            continue
        P = (H + 2 * pad - R) // stride + 1
        Q = (W + 2 * pad - S) // stride + 1
        M = N * P * Q
        assert M % 128 != 0
        tiles.add(M > 128)
        geo = (0, N, C, H, W, Ko, R, S, stride, pad)
        assert ext.conv2d_kloop_plan(*geo, 1) == "walk"
        assert ext.conv2d_kloop_plan(*geo, 0) == "decode"
        assert ext.conv2d_kloop_plan(*geo) == "walk"      # automatic: fit
        walk, dec = _fwd_pair(N, C, H, W, Ko, R, S, stride, pad, stats,
                              bias=Ko == 136)
        for a, b in zip(walk, dec):
            assert torch.equal(a, b), (N, C, H, W, Ko, stats)
    assert tiles


def test_forward_geometries_straddle_one_tile():
    """The row counts the forward cases run at lie on both sides of 128."""
    ms = {N * ((H + 2 * pad - R) // st + 1) * ((W + 2 * pad - S) // st + 1)
          for (N, H, W), (R, S), pad, st in itertools.product(
              GEOS, FILTERS, (0, 1, 2), (1, 2))}
    assert min(ms) < 128 < max(ms) and all(m % 128 for m in ms)


def _dgrad_pair(N, C, H, W, Ko, R, S, stride, pad, group, addend):
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    g = _gen("dgrad", N, C, H, W, Ko, R, S, stride, pad)
    dy = _act((N, Ko, P, Q), g)
    wt2 = torch.randn(C, R * S * Ko, device=DEV, generator=g).to(BF)
    add = _act((N, C, H, W), g) if addend else None
    return [ext.conv2d_dgrad(dy, wt2, N, C, H, W, R, S, stride, pad, add,
                             group, kwalk) for kwalk in (1, 0)]


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Ko", [64, 128, 192])
def test_dgrad_raster_walk_equals_decode(Ko, C, pad):
    for N, H, W in GEOS:
        geo = (1, N, C, H, W, Ko, 3, 3, 1, pad)
        assert ext.conv2d_kloop_plan(*geo, 1) == "walk"
        assert ext.conv2d_kloop_plan(*geo, 0) == "decode"
        assert ext.conv2d_kloop_plan(*geo) == "walk"
        walk, dec = _dgrad_pair(N, C, H, W, Ko, 3, 3, 1, pad, 0, False)
        assert torch.equal(walk, dec), (N, H, W)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Ko", [64, 128, 192])
def test_dgrad_taps_walk_equals_decode(Ko, C, pad):
    N, H, W = 32, 6, 7
    assert ext.conv2d_dgrad_plan(N, C, H, W, Ko, 3, 3, 1, pad, 32)[:2] \
        == ("taps", 32)
    assert ext.conv2d_kloop_plan(1, N, C, H, W, Ko, 3, 3, 1, pad, 1) == "walk"
    walk, dec = _dgrad_pair(N, C, H, W, Ko, 3, 3, 1, pad, 32, False)
    assert torch.equal(walk, dec)
    # and the tap-uniform walk against the raster decode loop
    raster = _dgrad_pair(N, C, H, W, Ko, 3, 3, 1, pad, 0, False)[1]
    assert torch.equal(walk, raster)


@pytest.mark.parametrize("group", [0, 32])
def test_dgrad_addend_walk_equals_decode(group):
    N, C, H, W, Ko, pad = 32, 128, 6, 7, 128, 1
    walk, dec = _dgrad_pair(N, C, H, W, Ko, 3, 3, 1, pad, group, True)
    assert torch.equal(walk, dec)


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("stats", [False, True])
def test_forward_fallback_is_decode(C, stats):
    for N, H, W in GEOS:
        geo = (0, N, C, H, W, 64, 3, 3, 1, 1)
        assert ext.conv2d_kloop_plan(*geo, 1) == "decode"
        assert ext.conv2d_kloop_plan(*geo) == "decode"
        walk, dec = _fwd_pair(N, C, H, W, 64, 3, 3, 1, 1, stats, bias=True)
        for a, b in zip(walk, dec):
            assert torch.equal(a, b)


def test_strided_dgrad_fallback_is_decode():
    for N, H, W in GEOS:
        geo = (1, N, 64, H, W, 128, 3, 3, 2, 1)
        assert ext.conv2d_kloop_plan(*geo, 1) == "decode"
        assert ext.conv2d_kloop_plan(*geo) == "decode"
        walk, dec = _dgrad_pair(N, 64, H, W, 128, 3, 3, 2, 1, -1, False)
        assert torch.equal(walk, dec)


def test_dgrad_odd_ko_fallback_is_decode():
    # Ko = 72: a K-tile would straddle taps
    N, H, W = GEOS[1]
    assert ext.conv2d_kloop_plan(1, N, 64, H, W, 72, 3, 3, 1, 1, 1) == "decode"
    walk, dec = _dgrad_pair(N, 64, H, W, 72, 3, 3, 1, 1, 0, False)
    assert torch.equal(walk, dec)


@pytest.mark.parametrize("name,mode,N,C,H,W,Ko,R,stride,pad", [
    ("conv2 fwd", 0, 1024, 64, 26, 26, 128, 3, 1, 0),
    ("conv3 fwd", 0, 1024, 128, 12, 12, 256, 3, 1, 0),
    ("conv4 fwd", 0, 1024, 256, 10, 10, 512, 3, 1, 0),
    ("conv2 dgrad", 1, 1024, 64, 26, 26, 128, 3, 1, 0),
    ("conv3 dgrad", 1, 1024, 128, 12, 12, 256, 3, 1, 0),
    ("conv4 dgrad", 1, 1024, 256, 10, 10, 512, 3, 1, 0),
    ("r18 3x3", 0, 256, 64, 32, 32, 64, 3, 1, 1),
    ("r18 3x3 dgrad", 1, 256, 64, 32, 32, 64, 3, 1, 1),
    ("r18 3x3/2", 0, 256, 64, 32, 32, 128, 3, 2, 1),
])
def test_automatic_rule_is_the_fit_rule(name, mode, N, C, H, W, Ko, R, stride,
                                        pad):
    """The measured shapes (the flagship's and the controls) run the walk."""
    assert ext.conv2d_kloop_plan(mode, N, C, H, W, Ko, R, R, stride, pad) \
        == "walk"


def test_tap_offset_past_int_is_decode():
    """(R*W + S)*C is the largest tap offset the kernel forms, in an int."""
    big = (2 ** 31) // (3 * 64) + 8                 # 3*W*64 just past 2^31
    assert ext.conv2d_kloop_plan(0, 1, 64, 8, big, 64, 3, 3, 1, 1, 1) \
        == "decode"
    assert ext.conv2d_kloop_plan(0, 1, 64, 8, big // 2, 64, 3, 3, 1, 1, 1) \
        == "walk"


def test_kwalk_argument_is_validated():
    with pytest.raises(RuntimeError):
        ext.conv2d_kloop_plan(0, 2, 64, 6, 6, 64, 3, 3, 1, 1, 2)
