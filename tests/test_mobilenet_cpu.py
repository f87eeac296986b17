"""MobileNetV1 and the grouped / dilated conv2d interface on the CPU tier."""
import pytest
import torch
import torch.nn.functional as TF

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops import modules as M_ops

BN_KEYS = ("weight", "bias", "running_mean", "running_var",
           "num_batches_tracked")


def test_parameter_count_and_state_dict_layout():
    m = build_model("mobilenet_v1")
    n = {k: p.numel() for k, p in m.named_parameters()}
    assert sum(n.values()) == 4_231_976
    assert n["conv1.weight"] == 864
    assert sum(v for k, v in n.items() if k.endswith(".dw.weight")) == 44_640
    assert sum(v for k, v in n.items() if k.endswith(".pw.weight")) == 3_139_584
    assert sum(v for k, v in n.items() if "bn" in k) == 21_888
    assert n["fc.weight"] + n["fc.bias"] == 1_025_000
    want = ["conv1.weight"] + [f"bn1.{k}" for k in BN_KEYS]
    for i in range(13):
        want += [f"blocks.{i}.dw.weight"]
        want += [f"blocks.{i}.bn_dw.{k}" for k in BN_KEYS]
        want += [f"blocks.{i}.pw.weight"]
        want += [f"blocks.{i}.bn_pw.{k}" for k in BN_KEYS]
    want += ["fc.weight", "fc.bias"]
    sd = m.state_dict()
    assert list(sd) == want
    assert sd["blocks.5.dw.weight"].shape == (256, 1, 3, 3)
    assert sd["blocks.5.pw.weight"].shape == (512, 256, 1, 1)
    assert m.blocks[5].dw.stride == (2, 2) and m.blocks[6].dw.stride == (1, 1)


def test_cifar_variant_forward_backward_on_cpu():
    torch.manual_seed(0)
    m = build_model("mobilenet_v1", num_classes=10, cifar_stem=True,
                    width_mult=0.25).train()
    assert m.fc.in_features == 256 and m.conv1.stride == (1, 1)
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10) and bool(out.isfinite().all())
    out.sum().backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(p.grad.isfinite().all()), k


@pytest.mark.parametrize("kw", [dict(padding=1, groups=8),
                                dict(padding=2, dilation=2),
                                dict(stride=2, groups=2, dilation=(2, 1))])
def test_grouped_and_dilated_modules_equal_torch_on_cpu(kw):
    torch.manual_seed(1)
    ours, ref = M_ops.Conv2d(8, 8, 3, **kw), torch.nn.Conv2d(8, 8, 3, **kw)
    ref.load_state_dict(ours.state_dict())
    x = torch.randn(2, 8, 9, 10)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ours(xa), ref(xb)
    assert torch.equal(ya, yb)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(ours.weight.grad, ref.weight.grad)


def test_dense_conv2d_on_cpu_is_unchanged():
    torch.manual_seed(2)
    x, w, b = torch.randn(2, 8, 9, 10), torch.randn(16, 8, 3, 3), torch.randn(16)
    want = TF.conv2d(x, w, b, 2, 1)
    assert torch.equal(F_ops.conv2d(x, w, b, 2, 1), want)
    assert torch.equal(F_ops.conv2d(x, w, b, 2, 1, groups=1), want)
    assert torch.equal(F_ops.conv2d(x, w, b, 2, 1, groups=1, dilation=1), want)
