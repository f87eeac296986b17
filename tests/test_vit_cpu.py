"""ViT-Ti / ViT-S structure and the CPU formulas of attention2d and the
sin-cos position table (no GPU)."""
import pytest
import torch

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops import modules as M_ops

F64 = torch.float64


@pytest.mark.parametrize("name,D,heads", [("vit_tiny", 192, 3),
                                          ("vit_small", 384, 6)])
def test_parameter_count_and_state_dict_layout(name, D, heads):
    m = build_model(name, num_classes=100)
    # patch conv; 12 blocks of qkv + proj + two pointwise (12 D^2) with their
    # biases, two norms and two layer scales (15 D); final norm; classifier
    want = (D * 3 * 16 * 16 + D) + 12 * (12 * D * D + 15 * D) + 2 * D \
        + (D * 100 + 100)
    assert sum(p.numel() for p in m.parameters()) == want
    per_block = ["norm1.weight", "norm1.bias", "attn.qkv.weight",
                 "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "ls1.gamma", "norm2.weight", "norm2.bias", "pw1.weight",
                 "pw1.bias", "pw2.weight", "pw2.bias", "ls2.gamma"]
    keys = (["patch.weight", "patch.bias"]
            + [f"blocks.{b}.{k}" for b in range(12) for k in per_block]
            + ["norm.weight", "norm.bias", "fc.weight", "fc.bias"])
    sd = m.state_dict()
    assert list(sd) == keys
    assert sd["blocks.3.attn.qkv.weight"].shape == (3 * D, D, 1, 1)
    assert m.blocks[0].attn.num_heads == heads
    assert bool((sd["blocks.11.ls2.gamma"] == 1e-4).all())


def test_forward_shape_and_finite_gradients_at_32x32():
    torch.manual_seed(1)
    m = build_model("vit_tiny", num_classes=10, cifar_stem=True)
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.square().sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(p.grad.isfinite().all()), name


def test_cpu_attention_is_the_float64_formula():
    g = torch.Generator().manual_seed(2)
    N, heads, H, W = 2, 3, 5, 13                     # L = 65
    qkv = torch.randn(N, 3 * 64 * heads, H, W, generator=g)
    rows = qkv.to(F64).permute(0, 2, 3, 1).reshape(N, H * W, 3, heads, 64)
    want = torch.empty(N, H * W, heads, 64, dtype=F64)
    for n in range(N):
        for h in range(heads):
            q, k, v = (rows[n, :, i, h] for i in range(3))
            want[n, :, h] = torch.softmax(q @ k.T / 8, dim=1) @ v
    got = F_ops.attention2d(qkv, heads)
    assert got.shape == (N, 64 * heads, H, W)
    torch.testing.assert_close(
        got.to(F64).permute(0, 2, 3, 1).reshape(N, H * W, heads, 64), want,
        rtol=0, atol=1e-5)


def test_pos_embed_is_the_sincos_formula_and_follows_the_grid():
    pe = M_ops.PosEmbed2d(16, 3, 5)
    assert "pos" not in pe.state_dict()
    x = torch.zeros(2, 16, 3, 5)
    y = pe(x)
    for i in range(4):
        om = 10000.0 ** (-i / 3)
        for (h, w) in [(0, 0), (2, 4), (1, 3)]:
            want = torch.tensor([w * om, h * om], dtype=F64)
            got = y[1, [i, 4 + i, 8 + i, 12 + i], h, w].to(F64)
            torch.testing.assert_close(
                got, torch.stack([want[0].sin(), want[0].cos(),
                                  want[1].sin(), want[1].cos()]),
                rtol=0, atol=1e-6)
    assert pe(torch.zeros(1, 16, 4, 2)).shape == (1, 16, 4, 2)
    assert pe.pos.shape == (1, 16, 4, 2)
