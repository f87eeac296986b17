"""FusedAdamW and FusedLAMB end to end on the GPU: six amp-O1 steps of
Toy_Net at B = 32 through Lookahead(optimizer(decay_param_groups(...)))
with gradient-norm clipping, run twice in fresh processes.  The third step
overflows (its loss scale is set to inf, so every gradient is non-finite):
the step is skipped on device and the step counters end at five."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
import torch
from ddp_tricks_amd import amp, same_seeds
from ddp_tricks_amd.models.toy_net import Toy_Net
from ddp_tricks_amd import ops
from ddp_tricks_amd.ops.functional import cross_entropy_loss
from ddp_tricks_amd.utils.lookahead import Lookahead

out_path, name = sys.argv[1], sys.argv[2]
ops.load_extension(required=True)
dev = torch.device("cuda:0")
same_seeds(42)
model = Toy_Net().to(dev)
cls = {"adamw": ops.FusedAdamW, "lamb": ops.FusedLAMB}[name]
opt = cls(ops.decay_param_groups(model, 0.05), lr=2e-3, betas=(0.9, 0.99),
          eps=1e-8, weight_decay=0.05)
la = Lookahead(opt, k=2, alpha=0.5)
model, la = amp.initialize(model, la, opt_level="O1", max_grad_norm=1.0)
g = torch.Generator().manual_seed(7)
x = torch.rand(32, 1, 28, 28, generator=g).to(dev)
t = torch.randint(0, 10, (32,), generator=g).to(dev)
model.train()
lazy, steps, ratios = [], [], []
for it in range(6):
    la.zero_grad()
    out = model(x)
    loss = cross_entropy_loss(out, t) / out.shape[0]
    scaler = amp.state().scaler
    keep = scaler.scale
    if it == 2:
        scaler.scale = float("inf")
    with amp.scale_loss(loss, la) as scaled:
        scaled.backward()
    scaler.scale = keep
    lazy.append(amp.pending_grad_scale() is not None)
    la.step()
    steps.append(opt._steps.clone())
    if name == "lamb":
        ratios.append(opt.trust_ratios.clone())
ordered = [p for grp in opt.param_groups for p in grp["params"]]
sd = la.state_dict()
torch.save({"params": {k: v.detach().cpu() for k, v in
                       model.state_dict().items()},
            "steps": torch.stack(steps).cpu(), "lazy": lazy,
            "ratios": torch.stack(ratios).cpu() if ratios else None,
            "ndim": [p.ndim for p in ordered],
            "state_keys": sorted(sd["fast_state"][0]),
            "state_step": float(sd["fast_state"][0]["step"]),
            "overflows": float(amp.state().overflow_count)}, out_path)
"""


def _run_child(tmp_path, name, tag):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / f"{name}_{tag}.pt")
    env = dict(os.environ)
    for k in ("DDPX_SYNC_AMP", "DDPX_CLIP_FUSED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _CHILD, out, name], cwd=repo,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["adamw", "lamb"])
def test_six_steps_with_one_overflow_repeat_bitwise(tmp_path, name):
    one = _run_child(tmp_path, name, "one")
    two = _run_child(tmp_path, name, "two")
    assert one["lazy"] == [True] * 6 and one["overflows"] == 1.0
    assert one["params"].keys() == two["params"].keys()
    for k in one["params"]:
        assert torch.equal(one["params"][k], two["params"][k]), k
        assert bool(torch.isfinite(one["params"][k]).all()), k
    n = len(one["ndim"])
    want = torch.tensor([1., 2., 2., 3., 4., 5.])     # the third is skipped
    assert torch.equal(one["steps"], want[:, None].expand(6, n))
    assert torch.equal(one["steps"], two["steps"])
    assert one["state_keys"] == ["exp_avg", "exp_avg_sq", "step"]
    assert one["state_step"] == 5.0
    ndim = torch.tensor(one["ndim"])
    assert int((ndim > 1).sum()) > 0 and int((ndim <= 1).sum()) > 0
    if name == "lamb":
        r = one["ratios"]                             # [steps, params]
        assert torch.equal(r, two["ratios"])
        assert r.shape == (6, n)
        adapted = r[:, ndim > 1]
        assert bool(torch.isfinite(adapted).all()) and bool(
            (adapted > 0).all())
        assert bool((r[:, ndim <= 1] == 1.0).all())
        assert torch.equal(r[1], r[2])                # the skipped step
        assert not torch.equal(r[0], r[5])
    else:
        assert one["ratios"] is None
