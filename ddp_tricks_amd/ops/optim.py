"""FusedSGD — nesterov-momentum SGD with a single multi-tensor step.

Replaces torch.optim.SGD in the reference recipe (reference
utils/train.py:41: SGD(lr, momentum=0.9, nesterov=True), stepped through
Lookahead).  On GPU the step is one fused multi-tensor HIP kernel over the
flattened param/grad/momentum lists; on CPU (and as the
reference oracle) the identical math runs via torch._foreach ops:

    buf = mu * buf + g            (no dampening, matches reference cfg)
    d   = g + mu * buf            (nesterov)
    p  -= lr * d

FusedLARS is the same step with a per-tensor trust ratio on the gradient
(layer-wise adaptive rate scaling, for large global batches); see its
docstring.
"""
from __future__ import annotations

from typing import List

import torch
from torch.optim import Optimizer


class FusedSGD(Optimizer):
    def __init__(self, params, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False):
        if lr < 0.0:
            raise ValueError(f"invalid lr {lr}")
        if nesterov and momentum <= 0:
            raise ValueError("nesterov momentum requires momentum > 0")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                        nesterov=nesterov)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            params: List[torch.Tensor] = []
            grads: List[torch.Tensor] = []
            bufs: List[torch.Tensor] = []
            momentum = group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                params.append(p)
                grads.append(p.grad)
                if momentum != 0:
                    state = self.state[p]
                    if "momentum_buffer" not in state:
                        state["momentum_buffer"] = torch.zeros_like(p)
                    bufs.append(state["momentum_buffer"])
            if not params:
                continue
            self._step_group(params, grads, bufs, group)
        return loss

    def _step_group(self, params, grads, bufs, group):
        lr, momentum = group["lr"], group["momentum"]
        wd, nesterov = group["weight_decay"], group["nesterov"]
        if params[0].is_cuda:
            from . import load_extension
            ext = load_extension(required=False)
            if ext is not None:
                from .. import amp as amp_mod
                ext.fused_sgd(params, grads, bufs, lr, momentum, wd,
                              1.0 if nesterov else 0.0,
                              amp_mod.pending_found_inf(),
                              amp_mod.pending_grad_scale())
                # raw-pointer writes don't bump Tensor._version — drop the
                # per-version bf16 weight cast cache so the next forward
                # re-casts the updated masters
                from .functional import clear_weight_cache
                clear_weight_cache()
                return
        if wd != 0:
            grads = torch._foreach_add(grads, params, alpha=wd)
        if momentum != 0:
            torch._foreach_mul_(bufs, momentum)
            torch._foreach_add_(bufs, grads)
            if nesterov:
                d = torch._foreach_add(grads, bufs, alpha=momentum)
            else:
                d = bufs
            torch._foreach_add_(params, d, alpha=-lr)
        else:
            torch._foreach_add_(params, grads, alpha=-lr)

    def zero_grad(self, set_to_none: bool = False):
        """Default zeros in place (NOT set-to-none): gradients are views
        into the DDP bucket flats and must keep their storage."""
        grads = [p.grad for g in self.param_groups for p in g["params"]
                 if p.grad is not None]
        if not grads:
            return
        if set_to_none:
            for g in self.param_groups:
                for p in g["params"]:
                    p.grad = None
        else:
            torch._foreach_zero_(grads)


class FusedLARS(Optimizer):
    """SGD with layer-wise adaptive rate scaling (the LARC "scale" formula).

    For every parameter tensor of a group with ``adapt=True``:

        g~  = g * gs                  (gs: pending lazy-clip coefficient)
        wn  = ||p||_2 ,  gn = ||g~||_2
        r   = eta * wn / (gn + wd * wn + eps)   if wn > 0 and gn > 0 else 1
        r   = min(r / lr, 1)                    with trust_clip (LARC clip)
        gi  = (g~ + wd * p) * r
        buf = mu * buf + gi ; d = nesterov ? gi + mu * buf : buf ; p -= lr * d

    Groups with ``adapt=False`` take exactly the ``FusedSGD`` update.  On
    GPU an adapted group is three multi-tensor HIP launches per 32 tensors
    (pair square sums, per-tensor ratio, step); no host sync, the amp
    overflow flag skips all of them on device.  On CPU (and as the oracle)
    the same formula runs in torch with the norms taken in float64.

    ``trust_ratios``: after a step, an fp32 tensor on the parameters'
    device with one ratio per parameter, in parameter order (1 for
    non-adapted parameters).  Allocated once and updated in place.  The
    optimizer state is the momentum buffers only.
    """

    def __init__(self, params, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False,
                 trust_coefficient: float = 0.001, eps: float = 1e-8,
                 trust_clip: bool = False):
        if lr < 0.0:
            raise ValueError(f"invalid lr {lr}")
        if nesterov and momentum <= 0:
            raise ValueError("nesterov momentum requires momentum > 0")
        if trust_coefficient <= 0.0:
            raise ValueError(f"invalid trust_coefficient {trust_coefficient}")
        if eps < 0.0:
            raise ValueError(f"invalid eps {eps}")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                        nesterov=nesterov, trust_coefficient=trust_coefficient,
                        eps=eps, trust_clip=trust_clip, adapt=True)
        super().__init__(params, defaults)
        self.trust_ratios = None
        self._partials = None

    def _ratio_buffer(self, device, count: int):
        tr = self.trust_ratios
        if tr is None or tr.device != device or tr.numel() != count:
            self.trust_ratios = torch.ones(count, dtype=torch.float32,
                                           device=device)
        return self.trust_ratios

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        count = sum(len(g["params"]) for g in self.param_groups)
        first = next((p for g in self.param_groups for p in g["params"]),
                     None)
        if first is None:
            return loss
        ratios = self._ratio_buffer(first.device, count)
        offset = 0
        for group in self.param_groups:
            momentum = group["momentum"]
            # runs of consecutive parameters that have a gradient: a run's
            # ratios are one contiguous slice of trust_ratios
            runs, run = [], None
            for i, p in enumerate(group["params"]):
                if p.grad is None:
                    run = None
                    continue
                if run is None:
                    run = (offset + i, [], [], [])
                    runs.append(run)
                run[1].append(p)
                run[2].append(p.grad)
                if momentum != 0:
                    state = self.state[p]
                    if "momentum_buffer" not in state:
                        state["momentum_buffer"] = torch.zeros_like(p)
                    run[3].append(state["momentum_buffer"])
            offset += len(group["params"])
            if not group["adapt"]:
                params = [p for r in runs for p in r[1]]
                if params:
                    FusedSGD._step_group(self, params,
                                         [g for r in runs for g in r[2]],
                                         [b for r in runs for b in r[3]],
                                         group)
                continue
            for start, params, grads, bufs in runs:
                self._step_adapted(params, grads, bufs, group,
                                   ratios[start:start + len(params)])
        return loss

    def _step_adapted(self, params, grads, bufs, group, ratios):
        lr, momentum = group["lr"], group["momentum"]
        wd, nesterov = group["weight_decay"], group["nesterov"]
        eta, eps = group["trust_coefficient"], group["eps"]
        trust_clip = group["trust_clip"]
        from . import require_ext_for
        ext = require_ext_for(params[0])
        if ext is not None:
            from .. import amp as amp_mod
            from .functional import clear_weight_cache, num_chunks
            need = 2 * max(1, num_chunks(params, ext))
            if (self._partials is None or self._partials.numel() < need
                    or self._partials.device != params[0].device):
                self._partials = torch.zeros(need, dtype=torch.float32,
                                             device=params[0].device)
            ext.fused_lars(params, grads, bufs, self._partials, ratios, lr,
                           momentum, wd, 1.0 if nesterov else 0.0, eta, eps,
                           bool(trust_clip), amp_mod.pending_found_inf(),
                           amp_mod.pending_grad_scale())
            # raw-pointer writes don't bump Tensor._version (see FusedSGD)
            clear_weight_cache()
            return
        # reference path: norms in float64, the update in fp32 foreach ops
        wn = torch.stack([torch.linalg.vector_norm(p.double())
                          for p in params])
        gn = torch.stack([torch.linalg.vector_norm(g.double())
                          for g in grads])
        r = eta * wn / (gn + wd * wn + eps)
        if trust_clip:
            r = torch.clamp(r / lr, max=1.0)
        r = torch.where((wn > 0) & (gn > 0), r, torch.ones_like(r))
        ratios.copy_(r)
        if wd != 0:
            grads = torch._foreach_add(grads, params, alpha=wd)
        grads = [g * r for g, r in zip(grads, ratios.unbind(0))]
        if momentum != 0:
            torch._foreach_mul_(bufs, momentum)
            torch._foreach_add_(bufs, grads)
            if nesterov:
                d = torch._foreach_add(grads, bufs, alpha=momentum)
            else:
                d = bufs
            torch._foreach_add_(params, d, alpha=-lr)
        else:
            torch._foreach_add_(params, grads, alpha=-lr)

    zero_grad = FusedSGD.zero_grad


def lars_param_groups(model, weight_decay: float = 0.0):
    """Two parameter groups for ``FusedLARS``: tensors with ``ndim <= 1``
    (BatchNorm scale and shift, biases) are neither adapted nor decayed;
    the rest are adapted and get ``weight_decay``.  Every trainable
    parameter lands in exactly one group; within a group the model's
    parameter order is kept."""
    adapted, plain = [], []
    for p in model.parameters():
        if not p.requires_grad:
            continue
        (plain if p.ndim <= 1 else adapted).append(p)
    return [
        dict(params=adapted, adapt=True, weight_decay=weight_decay),
        dict(params=plain, adapt=False, weight_decay=0.0),
    ]
