"""ConvNeXt-T's structure and the CPU formulas of layer_norm2d, gelu and
layer_scale (no GPU)."""
import math

import pytest
import torch

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops import modules as M_ops

F64 = torch.float64


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model("convnext_tiny")


def test_parameter_count_is_torchvisions(model):
    assert sum(p.numel() for p in model.parameters()) == 28_589_128


def test_depthwise_convs_are_7x7_at_the_four_widths(model):
    dw = [m for m in model.modules()
          if isinstance(m, M_ops.Conv2d) and m.groups > 1]
    assert len(dw) == 18
    assert all(m.kernel_size == (7, 7) and m.groups == m.in_channels
               and m.padding == (3, 3) and m.bias is not None for m in dw)
    assert {m.in_channels for m in dw} == {96, 192, 384, 768}


@pytest.mark.parametrize("cifar,size", [(False, 64), (True, 32)])
def test_forward_shape_and_finite_gradients(cifar, size):
    torch.manual_seed(1)
    m = build_model("convnext_tiny", num_classes=10, cifar_stem=cifar)
    out = m(torch.randn(2, 3, size, size))
    assert out.shape == (2, 10)
    out.square().sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(p.grad.isfinite().all()), name


def test_cpu_formulas_agree_with_float64():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 24, 3, 5, generator=g) + 0.5
    w, b = torch.randn(24, generator=g), torch.randn(24, generator=g)
    r = torch.randn(2, 24, 3, 5, generator=g)
    x6, w6, b6 = x.to(F64), w.to(F64).view(1, -1, 1, 1), b.to(F64).view(1, -1, 1, 1)
    mu = x6.mean(1, keepdim=True)
    var = (x6 - mu).square().mean(1, keepdim=True)
    ln = (x6 - mu) / (var + 1e-6).sqrt() * w6 + b6
    torch.testing.assert_close(F_ops.layer_norm2d(x, w, b).to(F64), ln,
                               rtol=0, atol=1e-5)
    ge = 0.5 * x6 * (1 + torch.erf(x6 / math.sqrt(2)))
    torch.testing.assert_close(F_ops.gelu(x).to(F64), ge, rtol=0, atol=1e-6)
    torch.testing.assert_close(F_ops.layer_scale(x, w, r).to(F64),
                               r.to(F64) + w6 * x6, rtol=0, atol=1e-6)
    assert torch.equal(M_ops.LayerScale(24)(x, r), r + 1e-6 * x)
