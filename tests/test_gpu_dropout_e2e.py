"""Fused dropout end to end on the GPU.

1. vgg16(num_classes=10, cifar_head=True, dropout=0.5) at B = 8, 32x32: six
   amp-O1 steps through Lookahead(FusedSGD), run in fresh processes.  Two
   runs of the same epoch are bitwise identical (loss and parameters); the
   same run under ``set_epoch(1)`` is not.
2. One training-mode forward of that model on the GPU and on the CPU draw
   the same masks: the zeros of both junctions' outputs are the numpy
   mirror's dropped elements.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
import torch
from ddp_tricks_amd import amp, ops, same_seeds
from ddp_tricks_amd.models import build_model
from ddp_tricks_amd.ops import FusedSGD, load_extension
from ddp_tricks_amd.ops.functional import cross_entropy_loss
from ddp_tricks_amd.utils.lookahead import Lookahead

out_path, epoch = sys.argv[1], int(sys.argv[2])
load_extension(required=True)
dev = torch.device("cuda:0")
same_seeds(42)
model = build_model("vgg16", num_classes=10, cifar_head=True,
                    dropout=0.5).to(dev)
opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, nesterov=True)
la = Lookahead(opt, k=2, alpha=0.5)
model, la = amp.initialize(model, la, opt_level="O1")
g = torch.Generator().manual_seed(7)
x = torch.rand(8, 3, 32, 32, generator=g).to(dev)
t = torch.randint(0, 10, (8,), generator=g).to(dev)
ops.dropout_rng.seed(42)
ops.dropout_rng.set_epoch(epoch)
model.train()
losses = []
for _ in range(6):
    la.zero_grad()
    out = model(x)
    loss = cross_entropy_loss(out, t) / out.shape[0]
    with amp.scale_loss(loss, la) as scaled:
        scaled.backward()
    la.step()
    losses.append(loss.detach().float().cpu())
torch.save({"params": {k: v.detach().cpu() for k, v in
                       model.state_dict().items()},
            "losses": torch.stack(losses),
            "calls": ops.dropout_rng.calls}, out_path)
"""


def _run_child(tmp_path, name, epoch):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / f"{name}.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, out, str(epoch)],
                       cwd=repo, env=dict(os.environ), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(400)
def test_six_dropout_steps_repeat_bitwise(tmp_path):
    one = _run_child(tmp_path, "one", 0)
    two = _run_child(tmp_path, "two", 0)
    other = _run_child(tmp_path, "other", 1)
    assert one["calls"] == two["calls"] == 12       # 2 junctions x 6 steps
    assert bool(torch.isfinite(one["losses"]).all())
    assert torch.equal(one["losses"], two["losses"])
    assert one["params"].keys() == two["params"].keys()
    for k in one["params"]:
        assert torch.equal(one["params"][k], two["params"][k]), k
        assert bool(torch.isfinite(one["params"][k].float()).all()), k
    # another epoch draws other masks: the run leaves other bits behind
    assert not torch.equal(one["losses"], other["losses"])
    assert any(not torch.equal(one["params"][k], other["params"][k])
               for k in one["params"])


def test_gpu_and_cpu_models_draw_the_same_masks(monkeypatch):
    """Both models' junction outputs are recorded through the helper the
    model calls.  With keep = the mirror's mask of that call:

    * every dropped element is exactly 0 on both devices;
    * CPU: the output is nonzero exactly where kept and the CPU
      pre-activation is positive;
    * GPU: the junction's pre-activation is re-evaluated in float64 from the
      junction's own bf16 input and the bf16-rounded weights the kernel
      reads.  The kernel's fp32 accumulation of K+1 terms differs from that
      by at most (K+1) * 2^-24 * sum|terms| (2x for slack), so wherever the
      float64 value is above that bound the element is active, and its
      zero/nonzero state must equal the mask.
    """
    from ddp_tricks_amd import ops, same_seeds
    from ddp_tricks_amd.models import build_model, vgg as vgg_mod
    from ddp_tricks_amd.ops import functional as Fo
    from ddp_tricks_amd.ops import load_extension
    load_extension(required=True)
    dev = torch.device("cuda:0")

    real = Fo.linear_relu_dropout
    rec = []

    def spy(lin_mod, drop_mod, x):
        y = real(lin_mod, drop_mod, x)
        rec.append((lin_mod, x.detach(), y.detach()))
        return y

    monkeypatch.setattr(vgg_mod, "linear_relu_dropout", spy)
    saved = ops.dropout_rng.state_dict()
    try:
        same_seeds(11)
        cpu = build_model("vgg16", num_classes=10, cifar_head=True,
                          dropout=0.5)
        gpu = build_model("vgg16", num_classes=10, cifar_head=True,
                          dropout=0.5)
        gpu.load_state_dict(cpu.state_dict())
        gpu = gpu.to(dev)
        g = torch.Generator().manual_seed(3)
        x = torch.rand(8, 3, 32, 32, generator=g)
        cpu.train()
        gpu.train()
        Fo.clear_weight_cache()
        ops.dropout_rng.seed(5, rank=0)
        ops.dropout_rng.set_epoch(2)
        with torch.no_grad():
            cpu(x)
        assert ops.dropout_rng.calls == 2
        ops.dropout_rng.set_epoch(2)
        with torch.no_grad():
            gpu(x.to(dev))
        assert ops.dropout_rng.calls == 2
        ops.dropout_rng.set_epoch(2)
        seeds = [ops.dropout_rng.next_call_seed() for _ in range(2)]
    finally:
        ops.dropout_rng.load_state_dict(saved)
        Fo.clear_weight_cache()

    assert len(rec) == 4
    thr = Fo.dropout_threshold(0.5)
    for j in range(2):
        lin_c, xin_c, y_c = rec[j]
        lin_g, xin_g, y_g = rec[2 + j]
        M, N = y_c.shape
        assert y_g.shape == (M, N) and y_g.dtype == torch.bfloat16
        keep = torch.from_numpy(Fo.dropout_mask(seeds[j], M * N, thr)) \
            .view(M, N)
        assert 0.4 < float(keep.float().mean()) < 0.6
        y_g = y_g.cpu()
        # dropped elements
        assert not bool(y_c[~keep].any()) and not bool(y_g[~keep].any())
        # CPU model: active == kept & positive pre-activation
        pre_c = torch.nn.functional.linear(xin_c, lin_c.weight, lin_c.bias)
        assert torch.equal(y_c != 0, keep & (pre_c > 0))
        # GPU model, on its own inputs
        xg = xin_g.cpu().to(torch.bfloat16).double()
        wg = lin_g.weight.detach().cpu().to(torch.bfloat16).double()
        bg = lin_g.bias.detach().cpu().double()
        pre_g = xg @ wg.t() + bg
        bound = 2.0 * (xg.shape[1] + 1) * 2.0 ** -24 \
            * (xg.abs() @ wg.abs().t() + bg.abs())
        sure = pre_g > bound
        assert int((sure & keep).sum()) > 0.1 * M * N
        assert torch.equal((y_g != 0)[sure], keep[sure])
        assert not bool(y_g[pre_g < -bound].any())
