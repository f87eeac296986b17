"""Squeeze-and-Excitation off the GPU: the torch formula, the module's keys
and the SE models' sizes."""
import pytest
import torch

from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.models.resnet import Bottleneck, resnet50
from ddp_tricks_amd.ops import SqueezeExcite

# SE adds 2 C (C/16) + C/16 + C per block on a Bottleneck's C = 4 * planes
SE_PARAMS = sum(b * (2 * c * (c // 16) + c // 16 + c)
                for b, c in zip((3, 4, 6, 3), (256, 512, 1024, 2048)))


def se64(u, w1, b1, w2, b2, r=None, relu=False):
    """The junction in float64, written out."""
    u, w1, b1, w2, b2 = (t.double() for t in (u, w1, b1, w2, b2))
    z = u.flatten(2).mean(2)
    h = (z @ w1.flatten(1).T + b1).clamp_min(0)
    s = 1 / (1 + torch.exp(-(h @ w2.flatten(1).T + b2)))
    y = u * s.view(s.shape + (1,) * (u.dim() - 2))
    if r is not None:
        y = y + r.double()
    return y.clamp_min(0) if relu else y


# C = 12 and a 3-D input are outside the kernels' scope on any device
@pytest.mark.parametrize("shape", [(2, 32, 5, 3), (3, 12, 4, 4), (2, 16, 7)])
@pytest.mark.parametrize("resid,relu", [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_cpu_formula_matches_float64(shape, resid, relu):
    g = torch.Generator().manual_seed(sum(shape) + 2 * resid + relu)
    se = SqueezeExcite(shape[1], reduction=4)
    u = torch.randn(shape, generator=g, requires_grad=True)
    r = torch.randn(shape, generator=g) if resid else None
    y = se(u, residual=r, fuse_relu=bool(relu))
    ps = [se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias]
    want = se64(u, *ps, r, relu)
    assert y.dtype == torch.float32 and y.shape == u.shape
    torch.testing.assert_close(y.double(), want, rtol=1e-5, atol=1e-6)
    dy = torch.randn(shape, generator=g)
    got = torch.autograd.grad(y, [u] + ps, dy)
    ref = torch.autograd.grad(want, [u] + ps, dy.double())
    for a, b in zip(got, ref):
        torch.testing.assert_close(a.double(), b.double(), rtol=1e-4,
                                   atol=1e-5)


def test_module_keys_and_shapes_are_timms():
    sd = SqueezeExcite(64, reduction=16).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "fc1.weight": (4, 64, 1, 1), "fc1.bias": (4,),
        "fc2.weight": (64, 4, 1, 1), "fc2.bias": (64,)}


def test_se_reduction_zero_is_todays_bottleneck():
    plain, zero = Bottleneck(64, 16), Bottleneck(64, 16, se_reduction=0)
    assert list(plain.state_dict()) == list(zero.state_dict())
    assert [type(m) for m in plain.modules()] == \
        [type(m) for m in zero.modules()]
    assert zero.bn3.fuse_relu and not hasattr(zero, "se")
    gated = Bottleneck(64, 16, se_reduction=16)
    assert not gated.bn3.fuse_relu and gated.bn1.fuse_relu
    assert set(gated.state_dict()) - set(plain.state_dict()) == {
        "se.fc1.weight", "se.fc1.bias", "se.fc2.weight", "se.fc2.bias"}
    x = torch.randn(2, 64, 5, 5, requires_grad=True)
    gated(x).square().mean().backward()
    assert bool(x.grad.isfinite().all())
    assert gated.se.fc1.weight.grad.abs().max() > 0


@pytest.mark.parametrize("name,base", [("se_resnet50", 25_557_032),
                                       ("se_resnext50_32x4d", 25_028_904)])
def test_registry_builds_the_se_models(name, base):
    assert SE_PARAMS == 2_530_992
    m = build_model(name)
    assert sum(p.numel() for p in m.parameters()) == base + SE_PARAMS
    sd = m.state_dict()
    assert sd["layer1.0.se.fc1.weight"].shape == (16, 256, 1, 1)
    assert sd["layer4.2.se.fc2.weight"].shape == (2048, 128, 1, 1)
    assert {k for k in sd if ".se." not in k} == set(resnet50().state_dict())

