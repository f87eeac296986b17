"""Carried rows of the wide wgrad kernels against a plain decode (no GPU).

conv2d_wgrad_walk_rows runs the same step function as the kernel's tile loop;
here its (n, p, q, valid) is compared with numpy's decode of
gm = (split + t*S)*DEPTH + row.
"""
import numpy as np
import pytest

from ddp_tricks_amd.ops import load_extension

ext = load_extension(required=True)

# (N, C, H, W, Ko, R, S, stride, pad, want_bias)
GEOMS = {
    "toy_conv2": (1024, 64, 26, 26, 128, 3, 3, 1, 0, True),
    "toy_conv3": (1024, 128, 12, 12, 256, 3, 3, 1, 0, True),
    "toy_conv4": (1024, 256, 10, 10, 512, 3, 3, 1, 0, True),
    "pq_divides_step_8x8": (64, 128, 10, 10, 128, 3, 3, 1, 0, False),
    "q70": (2, 128, 5, 72, 128, 3, 3, 1, 0, False),
    "q3": (40, 128, 5, 5, 128, 3, 3, 1, 0, True),
    "p1": (16, 128, 3, 40, 128, 3, 3, 1, 0, False),
    "s2_pad1_odd_h": (9, 128, 11, 13, 256, 3, 3, 2, 1, True),
    "n1": (1, 128, 30, 30, 128, 3, 3, 1, 1, False),
    "m_ragged": (3, 128, 13, 13, 128, 3, 3, 1, 0, True),
    "m_below_one_round": (1, 256, 6, 6, 512, 3, 3, 1, 0, False),
}


def _plan(g):
    leaf, S, _ = ext.conv2d_wgrad_plan(*g)
    assert leaf.startswith("wide_dma"), (g, leaf)
    return 64 if leaf == "wide_dma<64>" else 32, S


def _pq(g):
    N, C, H, W, Ko, R, S_, st, pad, _ = g
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S_) // st + 1


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_step_decomposition(name):
    g = GEOMS[name]
    depth, S = _plan(g)
    P, Q = _pq(g)
    loop, dn, dp, dq = ext.conv2d_wgrad_kloop_plan(*g, 1)
    assert loop == "walk"
    assert 0 <= dq < Q and 0 <= dp < P
    assert dn * P * Q + dp * Q + dq == S * depth
    assert ext.conv2d_wgrad_kloop_plan(*g, 0)[0] == "decode"


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_rows_match_decode(name):
    g = GEOMS[name]
    depth, S = _plan(g)
    P, Q = _pq(g)
    M = g[0] * P * Q
    tiles = -(-M // (S * depth)) + 1      # to the end of M and one beyond
    t = np.arange(tiles, dtype=np.int64)
    for split in sorted({0, min(1, S - 1), S - 1}):
        for row in (0, depth - 1):
            gm = (split + t * S) * depth + row
            want = np.stack([gm // (P * Q), gm // Q % P, gm % Q, gm < M], 1)
            got = np.array(ext.conv2d_wgrad_walk_rows(*g, split, row, tiles),
                           dtype=np.int64)
            assert np.array_equal(got, want), (name, split, row)


def test_m_below_one_round_has_invalid_rows():
    # M < S*DEPTH: the plan keeps eight tiles per split, so it reports S = 1
    # for so short an M, and the rows past M lie inside the only tile
    g = GEOMS["m_below_one_round"]
    depth, S = _plan(g)
    P, Q = _pq(g)
    M = g[0] * P * Q
    assert M < S * depth
    rows = ext.conv2d_wgrad_walk_rows(*g, S - 1, depth - 1, 2)
    assert [r[3] for r in rows] == [False, False]
    assert ext.conv2d_wgrad_walk_rows(*g, 0, M - 1, 1)[0][3] is True


def test_forced_walk_on_other_leaf_is_decode():
    g = (8, 64, 12, 12, 64, 3, 3, 1, 1, False)
    assert not ext.conv2d_wgrad_plan(*g)[0].startswith("wide_dma")
    assert ext.conv2d_wgrad_kloop_plan(*g, 1) == ("decode", 0, 0, 0)
    with pytest.raises(RuntimeError):
        ext.conv2d_wgrad_kloop_plan(*g, 2)
