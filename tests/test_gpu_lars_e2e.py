"""FusedLARS end to end on the GPU: six amp-O1 steps of Toy_Net at B = 32
through Lookahead(FusedLARS(lars_param_groups(...))) with gradient-norm
clipping, run twice in fresh processes."""
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
from ddp_tricks_amd.ops import FusedLARS, lars_param_groups, load_extension
from ddp_tricks_amd.ops.functional import cross_entropy_loss
from ddp_tricks_amd.utils.lookahead import Lookahead

out_path = sys.argv[1]
load_extension(required=True)
dev = torch.device("cuda:0")
same_seeds(42)
model = Toy_Net().to(dev)
opt = FusedLARS(lars_param_groups(model, 5e-4), lr=0.1, momentum=0.9,
                nesterov=True, trust_coefficient=0.02)
la = Lookahead(opt, k=2, alpha=0.5)
model, la = amp.initialize(model, la, opt_level="O1", max_grad_norm=1.0)
g = torch.Generator().manual_seed(7)
x = torch.rand(32, 1, 28, 28, generator=g).to(dev)
t = torch.randint(0, 10, (32,), generator=g).to(dev)
model.train()
lazy, ratios = [], []
for _ in range(6):
    la.zero_grad()
    out = model(x)
    loss = cross_entropy_loss(out, t) / out.shape[0]
    with amp.scale_loss(loss, la) as scaled:
        scaled.backward()
    lazy.append(amp.pending_grad_scale() is not None)
    la.step()
    ratios.append(opt.trust_ratios.clone())
ordered = [p for grp in opt.param_groups for p in grp["params"]]
torch.save({"params": {k: v.detach().cpu() for k, v in
                       model.state_dict().items()},
            "ratios": torch.stack(ratios).cpu(), "lazy": lazy,
            "ndim": [p.ndim for p in ordered],
            "overflows": float(amp.state().overflow_count)}, out_path)
"""


def _run_child(tmp_path, name):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / f"{name}.pt")
    env = dict(os.environ)
    for k in ("DDPX_SYNC_AMP", "DDPX_CLIP_FUSED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _CHILD, out], cwd=repo, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(300)
def test_six_lars_steps_repeat_bitwise(tmp_path):
    one = _run_child(tmp_path, "one")
    two = _run_child(tmp_path, "two")
    assert one["lazy"] == [True] * 6 and one["overflows"] == 0.0
    assert one["params"].keys() == two["params"].keys()
    for k in one["params"]:
        assert torch.equal(one["params"][k], two["params"][k]), k
        assert bool(torch.isfinite(one["params"][k]).all()), k
    assert torch.equal(one["ratios"], two["ratios"])
    ndim = torch.tensor(one["ndim"])
    assert int((ndim > 1).sum()) > 0 and int((ndim <= 1).sum()) > 0
    r = one["ratios"]                                  # [steps, params]
    assert r.shape == (6, len(one["ndim"]))
    adapted = r[:, ndim > 1]
    assert bool(torch.isfinite(adapted).all()) and bool((adapted > 0).all())
    assert bool((r[:, ndim <= 1] == 1.0).all())
    # the ratios are live: they move with the weights and the gradients
    assert not torch.equal(r[0], r[5])
