"""Carried-row wgrad loop (walk = 1) against the decode loop (walk = 0).

Both loops issue the same loads in the same order, so dw, and db where there
is a bias, must be bit-identical.  Shapes are the smallest that reach each
wide_dma leaf and each loop instantiation (pad 0 / pad > 0, bias / no bias).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ddp_tricks_amd.ops import load_extension
    ext = load_extension(required=True)
    DEV = torch.device("cuda:0")

D64, D32 = "wide_dma<64>", "wide_dma<32>"

# name: (N, C, H, W, Ko, R, S, leaf)
SHAPES = {
    "d64": (4, 128, 12, 12, 128, 3, 3, D64),
    "d32": (4, 64, 12, 12, 256, 3, 3, D32),
    "d64_ragged": (3, 128, 11, 11, 128, 3, 3, D64),
    "d32_ragged": (3, 64, 11, 11, 256, 3, 3, D32),
}
CASES = [(n, st, pad, bias) for n in SHAPES for st in (1, 2) for pad in (0, 1)
         for bias in (False, True)]
# name: (N, C, H, W, Ko, R, S, stride, pad, leaf)
EXTRA = {
    "out_8x8_step_is_images": (8, 128, 10, 10, 128, 3, 3, 1, 0, D64),
    "out_8x8_pad1": (8, 128, 8, 8, 128, 3, 3, 1, 1, D64),
    "out_8x8_d32": (8, 64, 10, 10, 256, 3, 3, 1, 0, D32),
    "out_8x8_d32_pad1": (8, 64, 8, 8, 256, 3, 3, 1, 1, D32),
    "out_8x8_s2_pad1": (8, 128, 16, 16, 128, 3, 3, 2, 1, D64),
    # four tiles only: the plan goes wide from M = 262144 rows
    "conv1x1_256": (256, 256, 32, 32, 256, 1, 1, 1, 0, D32),
    "ko192_partial_ko_tile": (4, 128, 12, 12, 192, 3, 3, 1, 1, D64),
    "ko192_pad0_ragged": (3, 128, 11, 11, 192, 3, 3, 1, 0, D64),
    "ko192_d32": (4, 64, 12, 12, 192, 3, 3, 1, 0, D32),
    "ko192_d32_s2_pad1_ragged": (3, 64, 11, 11, 192, 3, 3, 2, 1, D32),
    "c72_partial_rsc_tile": (4, 72, 12, 12, 256, 3, 3, 1, 0, D32),
    "c136_partial_rsc_tile": (4, 136, 12, 12, 128, 3, 3, 1, 1, D64),
    # conv2 has five tiles: sb_pair at N = 8 (both loops are decode), wide
    # from M = 262144 rows
    "toy_conv2_n8": (8, 64, 26, 26, 128, 3, 3, 1, 0, "sb_pair<32>"),
    "toy_conv2_n512": (512, 64, 26, 26, 128, 3, 3, 1, 0, D32),
    "toy_conv3_n8": (8, 128, 12, 12, 256, 3, 3, 1, 0, D64),
    "toy_conv4_n8": (8, 256, 10, 10, 512, 3, 3, 1, 0, D64),
}


def _check(N, C, H, W, Ko, R, S, stride, pad, leaf, bias):
    geom = (N, C, H, W, Ko, R, S, stride, pad, bias)
    assert ext.conv2d_wgrad_plan(*geom)[0] == leaf
    forced = "walk" if leaf in (D32, D64) else "decode"
    assert ext.conv2d_wgrad_kloop_plan(*geom, 1)[0] == forced
    assert ext.conv2d_wgrad_kloop_plan(*geom, 0)[0] == "decode"
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    g = torch.Generator(device=DEV)
    g.manual_seed(N * 1000003 + C * 1009 + Ko + H + pad)
    cl = torch.channels_last
    x = torch.randn(N, C, H, W, generator=g, device=DEV) \
        .to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(N, Ko, P, Q, generator=g, device=DEV) \
        .to(torch.bfloat16).contiguous(memory_format=cl)
    if bias:
        dw0, db0 = ext.conv2d_wgrad_bias(dy, x, R, S, stride, pad, 0)
        dw1, db1 = ext.conv2d_wgrad_bias(dy, x, R, S, stride, pad, 1)
        assert torch.equal(db0, db1)
    else:
        dw0 = ext.conv2d_wgrad(dy, x, R, S, stride, pad, 0)
        dw1 = ext.conv2d_wgrad(dy, x, R, S, stride, pad, 1)
    assert dw0.abs().max().item() > 0
    assert torch.equal(dw0, dw1)
    # the automatic plan runs one of the two
    dwa = ext.conv2d_wgrad(dy, x, R, S, stride, pad)
    assert torch.equal(dwa, dw0)


@pytest.mark.parametrize("name,stride,pad,bias", CASES)
def test_walk_equals_decode(name, stride, pad, bias):
    N, C, H, W, Ko, R, S, leaf = SHAPES[name]
    _check(N, C, H, W, Ko, R, S, stride, pad, leaf, bias)


@pytest.mark.parametrize("name", sorted(EXTRA))
@pytest.mark.parametrize("bias", [False, True])
def test_walk_equals_decode_extra(name, bias):
    _check(*EXTRA[name], bias)
