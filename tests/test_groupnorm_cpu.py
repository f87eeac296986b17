"""GroupNorm off the GPU: the converter, the CPU formula and the CLI flags."""
import importlib.util
import os
import sys

import pytest
import torch
import torch.nn.functional as TF

from ddp_tricks_amd import parallel
from ddp_tricks_amd.ops import functional as F_ops
from ddp_tricks_amd.ops.modules import (BatchNorm1d, BatchNorm2d, Conv2d,
                                        GroupNorm, Linear)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = Conv2d(1, 8, 3, padding=1)
        self.bn = BatchNorm2d(8, fuse_relu=True)
        self.fc = Linear(8 * 16, 8)
        self.bn1 = BatchNorm1d(8)

    def forward(self, x):
        x = F_ops.conv_bn(self.conv, self.bn, x)
        return self.bn1(self.fc(x.flatten(1)))


def test_convert_shares_parameters_drops_buffers_keeps_bn1d():
    torch.manual_seed(3)
    net = _Net()
    keys = set(net.state_dict())
    params = dict(net.named_parameters())
    out = parallel.convert_group_norm(net, num_groups=4)
    assert out is net
    assert isinstance(net.bn, GroupNorm) and net.bn.fuse_relu is True
    assert net.bn.num_groups == 4 and isinstance(net.bn1, BatchNorm1d)
    assert set(net.state_dict()) == keys - {
        "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}
    after = dict(net.named_parameters())
    assert after.keys() == params.keys()
    assert all(after[k] is params[k] for k in params)
    x = torch.randn(6, 1, 4, 4)
    want = TF.relu(TF.group_norm(net.conv(x), 4, net.bn.weight, net.bn.bias))
    assert torch.equal(F_ops.conv_bn(net.conv, net.bn, x), want)
    assert net(x).shape == (6, 8)
    root = parallel.convert_group_norm(BatchNorm2d(8), num_groups=8)
    assert isinstance(root, GroupNorm) and not root.fuse_relu
    with pytest.raises(ValueError, match="'bn'.*8 channels"):
        parallel.convert_group_norm(_Net(), num_groups=3)


@pytest.mark.parametrize("relu,resid", [(False, False), (True, False),
                                        (True, True)])
def test_cpu_group_norm_is_the_torch_formula(relu, resid):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 12, 3, 5, generator=g)
    w, b = torch.randn(12, generator=g), torch.randn(12, generator=g)
    r = torch.randn(2, 12, 3, 5, generator=g) if resid else None
    want = TF.group_norm(x, 3, w, b, 1e-5)
    if resid:
        want = want + r
    if relu:
        want = TF.relu(want)
    got = F_ops.group_norm(x, 3, w, b, 1e-5, fuse_relu=relu, residual=r)
    assert torch.equal(got, want)


def test_trainer_builds_bn_by_default_and_gn_on_request():
    import importlib
    import types
    from ddp_tricks_amd.models import build_model
    # (the package re-exports the train() function under the module's name)
    build = importlib.import_module(
        "ddp_tricks_amd.utils.train").build_train_model
    for args in (types.SimpleNamespace(), types.SimpleNamespace(norm="bn")):
        plain = build(args, "toy_net", {})
        assert not any(isinstance(m, GroupNorm) for m in plain.modules())
        assert list(plain.state_dict()) == list(
            build_model("toy_net").state_dict())
    gn = build(types.SimpleNamespace(norm="gn", gn_groups=16), "toy_net", {})
    assert sum(isinstance(m, GroupNorm) for m in gn.modules()) == 4
    assert not any(isinstance(m, BatchNorm2d) for m in gn.modules())
    with pytest.raises(ValueError, match="exclude"):
        build(types.SimpleNamespace(norm="gn", sync_bn=True), "toy_net", {})


def _load_run():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "_run_cli_gn", os.path.join(repo, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_norm_flags(monkeypatch):
    run = _load_run()
    monkeypatch.setattr(sys, "argv", ["run.py"])
    args = run.parse_args()
    assert args.norm == "bn" and args.gn_groups == 32
    monkeypatch.setattr(sys, "argv", ["run.py", "--norm", "gn",
                                      "--gn_groups", "8"])
    args = run.parse_args()
    assert args.norm == "gn" and args.gn_groups == 8
    monkeypatch.setattr(sys, "argv", ["run.py", "--norm", "gn", "--sync_bn"])
    with pytest.raises(SystemExit):
        run.parse_args()
