"""MnasNet-B1 (models/mnasnet.py) on the CPU path: structure, shapes and that
every parameter takes part in the backward."""
import torch

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.models.mnasnet import mnasnet1_0


def test_parameter_count_and_depthwise_kernel_sizes():
    model = mnasnet1_0()
    assert sum(p.numel() for p in model.parameters()) == 4_383_312
    assert tuple(stack[0].dw.kernel_size[0] for stack in model.stacks) == \
        (3, 5, 5, 3, 5, 3)
    wide = sorted({b.dw.in_channels for s in model.stacks for b in s
                   if b.dw.kernel_size == (5, 5)})
    assert wide == [72, 120, 240, 480, 576, 1152]


def test_forward_shapes_and_every_parameter_gets_a_gradient():
    torch.manual_seed(0)
    model = build_model("mnasnet1_0").train()
    out = model(torch.randn(2, 3, 64, 64))
    assert out.shape == (2, 1000)
    out.sum().backward()
    assert all(p.grad is not None and bool(p.grad.isfinite().all())
               for p in model.parameters())
    small = build_model("mnasnet1_0", num_classes=10, cifar_stem=True).train()
    assert small(torch.randn(2, 3, 32, 32)).shape == (2, 10)
