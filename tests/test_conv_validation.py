"""Conv2d stride/padding handling off the GPU: tuples reach the torch
fallback unchanged, and the HIP path's uniformity rule is enforced by a
helper that never silently drops the second element."""
import pytest
import torch

from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops.modules import Conv2d


@pytest.mark.parametrize("cfg", [
    dict(kernel_size=(1, 3), padding=(0, 1)),
    dict(kernel_size=(3, 1), padding=(1, 0), stride=(2, 1)),
    dict(kernel_size=3, padding=(2, 1), stride=(1, 2)),
    dict(kernel_size=3, padding=1, stride=2),
])
def test_conv2d_module_matches_torch_non_uniform(cfg):
    torch.manual_seed(0)
    ours = Conv2d(8, 8, **cfg)
    ref = torch.nn.Conv2d(8, 8, **cfg)
    ref.load_state_dict(ours.state_dict())
    x = torch.randn(2, 8, 9, 11)
    y, yr = ours(x), ref(x)
    assert y.shape == yr.shape
    assert torch.equal(y, yr)


def test_functional_conv2d_passes_tuples_through():
    torch.manual_seed(1)
    x = torch.randn(2, 4, 7, 9)
    w = torch.randn(6, 4, 1, 3)
    y = F_ops.conv2d(x, w, None, stride=(1, 1), padding=(0, 1))
    assert y.shape == (2, 6, 7, 9)
    assert torch.equal(y, torch.nn.functional.conv2d(x, w, None, (1, 1),
                                                     (0, 1)))


def test_uniform_reduces_or_raises():
    assert F_ops._uniform(2, "stride") == 2
    assert F_ops._uniform((1, 1), "stride") == 1
    assert F_ops._uniform([3, 3], "padding") == 3
    with pytest.raises(ValueError):
        F_ops._uniform((0, 1), "padding")
    with pytest.raises(ValueError):
        F_ops._uniform((1, 2), "stride")
