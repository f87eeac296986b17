"""ResNeXt on the shared Bottleneck: sizes, key names, a CPU step."""
import torch

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.models.resnet import resnet50, resnext50_32x4d


def _bottleneck_params(layers, groups, base_width, num_classes=1000):
    """Parameter count of a torchvision-rule bottleneck ResNet by formula."""
    total = 3 * 64 * 49 + 2 * 64                      # stem conv + bn
    inplanes = 64
    for i, (planes, blocks) in enumerate(zip((64, 128, 256, 512), layers)):
        width = int(planes * base_width / 64) * groups
        out = planes * 4
        for b in range(blocks):
            total += inplanes * width + 2 * width                 # conv1, bn1
            total += width * (width // groups) * 9 + 2 * width    # conv2, bn2
            total += width * out + 2 * out                        # conv3, bn3
            if b == 0:                        # every first block downsamples
                total += inplanes * out + 2 * out
            inplanes = out
    return total + 2048 * num_classes + num_classes


def test_resnext50_parameter_count():
    assert _bottleneck_params((3, 4, 6, 3), 32, 4) == 25_028_904
    n = sum(p.numel() for p in resnext50_32x4d().parameters())
    assert n == 25_028_904


def test_state_dict_keys_equal_resnet50s_and_resnet50_is_unchanged():
    r50, x50 = resnet50().state_dict(), resnext50_32x4d().state_dict()
    assert set(r50) == set(x50)
    assert sum(v.numel() for k, v in r50.items()
               if "num_batches" not in k and "running" not in k) == \
        _bottleneck_params((3, 4, 6, 3), 1, 64) == 25_557_032
    assert r50["layer1.0.conv2.weight"].shape == (64, 64, 3, 3)
    assert r50["layer4.2.conv2.weight"].shape == (512, 512, 3, 3)
    assert x50["layer1.0.conv2.weight"].shape == (128, 4, 3, 3)
    assert x50["layer4.2.conv2.weight"].shape == (1024, 32, 3, 3)
    x101 = build_model("resnext101_32x8d").state_dict()
    assert x101["layer3.22.conv2.weight"].shape == (1024, 32, 3, 3)
    assert x101["layer4.0.conv2.weight"].shape == (2048, 64, 3, 3)


def test_cpu_forward_backward_is_finite():
    torch.manual_seed(0)
    m = build_model("resnext50_32x4d", num_classes=10, cifar_stem=True)
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.square().mean().backward()
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and bool(g.isfinite().all()) for g in grads)
    assert m.layer1[0].conv2.weight.grad.abs().max() > 0
