"""Label smoothing + CutMix end to end on the GPU: six amp + FusedSGD steps
of Toy_Net at B = 64 on one fixed CutMix batch from the batch kernel."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 6


def _run(seed=42):
    from ddp_tricks_amd import amp, same_seeds
    from ddp_tricks_amd.models.toy_net import Toy_Net
    from ddp_tricks_amd.ops import MixedTarget, cross_entropy_loss
    from ddp_tricks_amd.ops.optim import FusedSGD
    from ddp_tricks_amd.utils.data import MNIST, Augment, DeviceBatchLoader
    device = torch.device("cuda:0")
    amp._state.__init__()
    same_seeds(seed)
    ds = MNIST(root="/nonexistent", train=True, synthetic=True, num_samples=64)
    loader = DeviceBatchLoader(ds, 64, device=device, seed=seed,
                               augment=Augment(hflip=True, cutmix_prob=1.0))
    (image, target), = list(loader)
    assert isinstance(target, MixedTarget)
    assert bool((target.lam < 1).any()) and bool((target.a != target.b).any())
    model = Toy_Net().to(device)
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, nesterov=True)
    model, opt = amp.initialize(model, opt, opt_level="O1")
    model.train()
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        out = model(image)
        loss = cross_entropy_loss(out, target, label_smoothing=0.1)
        with amp.scale_loss(loss / out.shape[0], opt) as scaled:
            scaled.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in model.parameters()]
    amp._state.__init__()
    return [float(l) for l in losses], losses, params


def test_six_steps_learn_and_repeat_bitwise():
    vals, losses, params = _run()
    print("losses:", " ".join(f"{v:.5f}" for v in vals))
    assert all(math.isfinite(v) for v in vals)
    assert vals[-1] < vals[0]
    _, losses2, params2 = _run()
    for a, b in zip(losses, losses2):
        assert torch.equal(a, b)
    for a, b in zip(params, params2):
        assert torch.equal(a, b)
