"""Tap-uniform row order of the stride-1 conv dgrad (`conv2d_dgrad(...,
group=G)`, `conv2d_dgrad_plan`; docs/KERNELS.md "Dgrad: tap-uniform rows").

With group = G the GEMM rows run (image group, pixel, image in group), so a
128-row tile holds 128/G dx pixels of G images and the K loop steps over the
taps that no pixel of the tile reaches.  Every case checks

(a) dx on the integer inputs of tests/test_gpu_exact.py (dy in {-2..2},
    weights in {-1, 0, 1}) against the float64 CPU reference rounded once to
    bf16, by ``torch.equal``; the 2^24 precondition is asserted on the
    reference alone;
(b) on random bf16 data, group = G against group = 0 by ``torch.equal``: the
    K-tiles that remain run in the raster kernel's order and a skipped one
    only added 0 * w;
(c) the (name, G) that ``conv2d_dgrad_plan`` reports for the forced G;
(d) ``k_tiles_issued`` against a count made here from the definition: per
    128-row tile, the union over the tile's pixels of the taps (r, s) with
    0 <= h + pad - r < P and 0 <= w + pad - s < Q, the whole image for a
    tile that crosses an image-group boundary, times Ko/64.

Shapes are (N, C, H, W, Ko, R, S, pad, G), stride 1.  All tests
@pytest.mark.gpu.
"""
import functools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

BF = torch.bfloat16
EXACT_LIMIT = float(2 ** 24)
TILE_M = 128


def _ints(shape, lo, hi, *key):
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, lo, hi) + key)
                                                 .encode()))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _act(t):
    return _nhwc(t.to(BF)).to(DEV)


def _wt2(w):
    K, C, R, S = w.shape
    return w.to(BF).permute(1, 2, 3, 0).reshape(C, R * S * K) \
        .contiguous().to(DEV)


def _bf16_round(ref64):
    return ref64.to(torch.float32).to(BF)


@functools.lru_cache(maxsize=None)
def _case(N, C, H, W, K, R, S, stride, pad):
    """Integer dy, w, float64 dx and the sum of |terms|; random bf16 dy, w."""
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    dy = _ints((N, K, P, Q), -2, 2, "dy")
    w = _ints((K, C, R, S), -1, 1, "w")
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w, dy, stride=stride,
                                     padding=pad)
    absref = torch.nn.grad.conv2d_input((N, C, H, W), w.abs(), dy.abs(),
                                        stride=stride, padding=pad)
    g = torch.Generator().manual_seed(zlib.crc32(repr((N, C, H, W, K, R, S))
                                                 .encode()))
    rdy = torch.randn((N, K, P, Q), generator=g).to(BF)
    rw = torch.randn((K, C, R, S), generator=g).to(BF)
    return dy, w, ref, absref, rdy, rw


def _model_taps(N, H, W, R, S, pad, G):
    """(M-tiles, taps issued, taps of all tiles) from the definition."""
    P, Q = H + 2 * pad - R + 1, W + 2 * pad - S + 1
    M = N * H * W
    ghw = G * H * W
    tiles = (M + TILE_M - 1) // TILE_M
    issued = 0
    for t in range(tiles):
        rows = range(t * TILE_M, min((t + 1) * TILE_M, M))
        groups = {m // ghw for m in rows}
        pixels = {(m % ghw) // G for m in rows}
        if len(groups) > 1:
            pixels = set(range(H * W))
        taps = set()
        for pix in pixels:
            h, wc = divmod(pix, W)
            for r in range(R):
                for s in range(S):
                    if 0 <= h + pad - r < P and 0 <= wc + pad - s < Q:
                        taps.add((r, s))
        issued += len(taps)
    return tiles, issued, tiles * R * S


# shape, then (M-tiles, taps issued, taps of all tiles) where the counts were
# worked out independently of this file's model
TAPS_CASES = [
    # one pixel per tile, 64-wide column tile, tiles of 1, 2 and 4 taps
    ((128, 8, 4, 4, 64, 3, 3, 0, 128), (16, 36, 144)),
    # every tile exactly one tap
    ((128, 8, 3, 3, 64, 3, 3, 0, 128), (9, 9, 81)),
    # four pixels per tile crossing image rows, 128-wide tile, two K-tiles
    # per tap, partial last tile (800 rows)
    ((32, 128, 5, 5, 128, 3, 3, 0, 32), (7, 36, 63)),
    # H != W, R != S
    ((64, 16, 6, 5, 64, 3, 2, 0, 64), (15, 60, 90)),
    # padding
    ((32, 8, 6, 6, 64, 3, 3, 1, 32), (9, 75, 81)),
    # G*H*W = 288 is no multiple of 128: a tile crosses a group boundary
    ((64, 8, 3, 3, 64, 3, 3, 0, 32), None),
    # partial second column tile (C = 64 + 8)
    ((32, 72, 5, 5, 64, 3, 3, 0, 32), None),
    # 25 taps, dy 2x2
    ((32, 8, 6, 6, 64, 5, 5, 0, 32), None),
    # 16 M-tiles of four pixels: a multiple of 8, the XCD tile walk
    ((32, 8, 8, 8, 64, 3, 3, 0, 32), None),
]


@pytest.mark.parametrize("shape,counts", TAPS_CASES)
def test_dgrad_taps(shape, counts):
    N, C, H, W, K, R, S, pad, G = shape
    dy, w, ref, absref, rdy, rw = _case(N, C, H, W, K, R, S, 1, pad)
    assert absref.abs().max().item() < EXACT_LIMIT

    # (c), (d): the plan, and its K-tile count against the model
    tiles, issued, all_taps = _model_taps(N, H, W, R, S, pad, G)
    if counts is not None:
        assert (tiles, issued, all_taps) == counts
    name, g, k_issued, k_raster = ext.conv2d_dgrad_plan(
        N, C, H, W, K, R, S, 1, pad, G)
    print(f"plan {name} G={g} k_tiles {k_issued}/{k_raster}; model "
          f"{issued * (K // 64)}/{all_taps * (K // 64)}")
    assert (name, g) == ("taps", G)
    assert k_raster == all_taps * (K // 64)
    assert k_issued == issued * (K // 64)
    assert issued < all_taps

    # (a) exact
    dx = ext.conv2d_dgrad(_act(dy), _wt2(w), N, C, H, W, R, S, 1, pad,
                          None, G)
    assert dx.shape == ref.shape and dx.dtype == BF
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(dx.cpu(), _bf16_round(ref))

    # (b) bit-identical to the raster order on random data
    a, b = _act(rdy), _wt2(rw)
    dx0 = ext.conv2d_dgrad(a, b, N, C, H, W, R, S, 1, pad, None, 0)
    dxg = ext.conv2d_dgrad(a, b, N, C, H, W, R, S, 1, pad, None, G)
    assert torch.equal(dxg.cpu().view(torch.int16),
                       dx0.cpu().view(torch.int16))


def test_dgrad_taps_addin():
    """Case 3 with the fused addend: dx + addin, rounded as the raster
    kernel rounds it (bf16(float(bf16(ref)) + g)), read at the permuted
    row's physical address."""
    (N, C, H, W, K, R, S, pad, G), _ = TAPS_CASES[2]
    dy, w, ref, absref, rdy, rw = _case(N, C, H, W, K, R, S, 1, pad)
    assert absref.abs().max().item() < EXACT_LIMIT
    assert ext.conv2d_dgrad_plan(N, C, H, W, K, R, S, 1, pad, G)[:2] == \
        ("taps", G)
    # even integers up to 256 are exact in bf16 and push sums onto ties
    g = _ints((N, C, H, W), -128, 128, "addend") * 2
    assert torch.equal(g.to(BF).double(), g)
    want = (_bf16_round(ref).float() + g.float()).to(BF)
    dx = ext.conv2d_dgrad(_act(dy), _wt2(w), N, C, H, W, R, S, 1, pad,
                          _act(g), G)
    assert torch.equal(dx.cpu(), want)
    a, b = _act(rdy), _wt2(rw)
    add = _act(torch.randn((N, C, H, W),
                           generator=torch.Generator().manual_seed(7)))
    dx0 = ext.conv2d_dgrad(a, b, N, C, H, W, R, S, 1, pad, add, 0)
    dxg = ext.conv2d_dgrad(a, b, N, C, H, W, R, S, 1, pad, add, G)
    assert torch.equal(dxg.cpu().view(torch.int16),
                       dx0.cpu().view(torch.int16))


# (N, C, H, W, Ko, R, S, stride, pad, forced G): shapes the tap-uniform order
# does not fit run raster, and the plan says so
FALLBACK_CASES = [
    (32, 8, 5, 5, 72, 3, 3, 1, 0, 32),    # Ko = 72: a K-tile straddles taps
    (48, 8, 5, 5, 64, 3, 3, 1, 0, 32),    # N = 48 is no multiple of G = 32
    (32, 8, 6, 6, 64, 3, 3, 2, 0, 32),    # stride 2
    (32, 8, 5, 5, 64, 1, 1, 1, 0, 32),    # 1x1: nothing to skip
]


@pytest.mark.parametrize("shape", FALLBACK_CASES)
def test_dgrad_taps_fallback_is_raster(shape):
    N, C, H, W, K, R, S, stride, pad, G = shape
    dy, w, ref, absref, _, _ = _case(N, C, H, W, K, R, S, stride, pad)
    assert absref.abs().max().item() < EXACT_LIMIT
    name, g, k_issued, k_raster = ext.conv2d_dgrad_plan(
        N, C, H, W, K, R, S, stride, pad, G)
    assert (name, g) == ("raster", 0)
    assert k_issued == k_raster
    dx = ext.conv2d_dgrad(_act(dy), _wt2(w), N, C, H, W, R, S, stride, pad,
                          None, G)
    assert torch.equal(dx.cpu(), _bf16_round(ref))


def test_dgrad_rejects_unknown_group():
    with pytest.raises(RuntimeError):
        ext.conv2d_dgrad_plan(32, 8, 5, 5, 64, 3, 3, 1, 0, 16)


# the automatic plan at the three Toy_Net dgrad shapes, B = 1024: what the
# micro-benchmark routed (docs/KERNELS.md, per-shape table)
TOYNET_AUTO = [
    ((1024, 64, 26, 26, 128, 3, 3, 1, 0), ("raster", 0)),     # conv2
    ((1024, 128, 12, 12, 256, 3, 3, 1, 0), ("taps", 128)),    # conv3
    ((1024, 256, 10, 10, 512, 3, 3, 1, 0), ("taps", 128)),    # conv4
]


@pytest.mark.parametrize("shape,want", TOYNET_AUTO)
def test_dgrad_auto_plan_toynet(shape, want):
    assert ext.conv2d_dgrad_plan(*shape)[:2] == want
    assert ext.conv2d_dgrad_plan(*shape, -1)[:2] == want
