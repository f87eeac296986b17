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
docstring.  FusedAdamW and FusedLAMB are the Adam-class steps on the same
multi-tensor path, with a device-side step counter so that the amp overflow
skip does not advance the bias correction.
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


ADAM_NCOEF = 4      # floats per tensor in the coefficient flat (elementwise.hip)


class _FusedAdamBase(Optimizer):
    """What FusedAdamW and FusedLAMB share: the step-counter flat, the
    moment state and the AdamW step.

    ``_steps`` is one fp32 tensor ``[n_params]`` on the parameters' device,
    in parameter order; ``state[p]["step"]`` is a 0-dim view of its entry,
    so the per-parameter state has torch's names and meaning (``step``,
    ``exp_avg``, ``exp_avg_sq``) while the kernels advance all counters of
    a launch group at once, on device, and only when the amp overflow flag
    is clear.  ``_coefs`` holds the bias-correction coefficients the tick
    kernel writes for the step kernels (``ADAM_NCOEF`` per parameter).
    """

    def _init_flats(self):
        self._steps = None
        self._coefs = None

    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _rebuild_flats(self, device):
        """New flats on ``device``; ``step`` values already in the state
        (a loaded or transplanted state dict) are folded in and re-pointed
        at their entries."""
        params = self._all_params()
        steps = torch.zeros(len(params), dtype=torch.float32, device=device)
        idx, vals = [], []
        for i, p in enumerate(params):
            if p in self.state and "step" in self.state[p]:
                idx.append(i)
                vals.append(torch.as_tensor(self.state[p]["step"]).detach()
                            .to(device=device, dtype=torch.float32)
                            .reshape(()))
        if idx:
            steps[idx] = torch.stack(vals)
        self._steps = steps
        self._coefs = torch.zeros(ADAM_NCOEF * len(params),
                                  dtype=torch.float32, device=device)
        for i in idx:
            self.state[params[i]]["step"] = steps[i]

    def _flats(self, device):
        count = sum(len(g["params"]) for g in self.param_groups)
        s = self._steps
        if s is None or s.device != device or s.numel() != count:
            self._rebuild_flats(device)
        return self._steps, self._coefs

    def _runs(self, group, offset, steps):
        """Runs of consecutive parameters that have a gradient, as
        (start, params, grads, exp_avgs, exp_avg_sqs): a run's counters are
        one contiguous slice of the flat.  Parameters without a gradient
        are skipped and their ``step`` does not advance."""
        runs, run = [], None
        for i, p in enumerate(group["params"]):
            if p.grad is None:
                run = None
                continue
            if run is None:
                run = (offset + i, [], [], [], [])
                runs.append(run)
            state = self.state[p]
            if "exp_avg" not in state:
                state["step"] = steps[offset + i]
                state["exp_avg"] = torch.zeros_like(p)
                state["exp_avg_sq"] = torch.zeros_like(p)
            run[1].append(p)
            run[2].append(p.grad)
            run[3].append(state["exp_avg"])
            run[4].append(state["exp_avg_sq"])
        return runs

    def _adamw_run(self, run, group, decoupled):
        start, params, grads, ms, vs = run
        n = len(params)
        lr, (b1, b2) = group["lr"], group["betas"]
        eps, wd = group["eps"], group["weight_decay"]
        steps = self._steps[start:start + n]
        from . import require_ext_for
        ext = require_ext_for(params[0])
        if ext is not None:
            from .. import amp as amp_mod
            from .functional import clear_weight_cache
            coefs = self._coefs[ADAM_NCOEF * start:ADAM_NCOEF * (start + n)]
            ext.fused_adamw(params, grads, ms, vs, steps, coefs, lr, b1, b2,
                            eps, wd, bool(decoupled),
                            amp_mod.pending_found_inf(),
                            amp_mod.pending_grad_scale())
            # raw-pointer writes don't bump Tensor._version (see FusedSGD)
            clear_weight_cache()
            return
        # reference path: the same formula in fp32 torch ops
        steps.add_(1)
        for p, g, m, v, s in zip(params, grads, ms, vs, steps.tolist()):
            bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
            if not decoupled and wd != 0:
                g = g.add(p, alpha=wd)
            _moments(g, m, v, b1, b2)
            if decoupled and wd != 0:
                p.mul_(1.0 - lr * wd)
            denom = (v.sqrt() / bc2 ** 0.5).add_(eps)
            p.addcdiv_(m, denom, value=-(lr / bc1))

    def state_dict(self):
        """torch's layout; every ``step`` is a clone of its entry of the
        flat (a device copy, no host sync), never a view that would drag
        the whole flat into a checkpoint."""
        sd = super().state_dict()
        sd["state"] = {
            k: {n: (v.clone() if n == "step" else v) for n, v in st.items()}
            for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        params = self._all_params()
        if params:
            self._rebuild_flats(params[0].device)

    zero_grad = FusedSGD.zero_grad


def _moments(g, m, v, b1, b2):
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    v.mul_(b2).addcmul_(g, g, value=1.0 - b2)


def _check_adam_args(lr, betas, eps, weight_decay):
    if lr < 0.0:
        raise ValueError(f"invalid lr {lr}")
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"invalid betas {betas}")
    if eps < 0.0:
        raise ValueError(f"invalid eps {eps}")
    if weight_decay < 0.0:
        raise ValueError(f"invalid weight_decay {weight_decay}")


class FusedAdamW(_FusedAdamBase):
    """AdamW (``decoupled=False``: Adam with L2 decay) in torch's formula:

        g~ = g * gs                   (gs: pending lazy-clip coefficient)
        g~ = g~ + wd * p              (decoupled=False only)
        m  = b1 * m + (1 - b1) * g~
        v  = b2 * v + (1 - b2) * g~ * g~
        p  = p * (1 - lr * wd)        (decoupled=True only)
        p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
        bc1 = 1 - b1^step, bc2 = 1 - b2^step

    On GPU a step is two HIP launches per 32 tensors: a tick that advances
    the per-parameter step counters and writes the bias-correction
    coefficients on device, and one pass over g, p, m, v.  No host sync and
    no per-step H2D copy; when the amp overflow flag is set both launches
    are no-ops, so a skipped step does not advance the bias correction.  On
    CPU (and as the oracle) the same formula runs in torch ops.

    The state is torch's (``step`` as a 0-dim fp32 tensor, ``exp_avg``,
    ``exp_avg_sq``): ``state_dict()["state"]`` can be loaded into
    ``torch.optim.AdamW`` and the other way round.
    """

    def __init__(self, params, lr: float, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.01,
                 decoupled: bool = True):
        _check_adam_args(lr, betas, eps, weight_decay)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps,
                        weight_decay=weight_decay, decoupled=bool(decoupled))
        super().__init__(params, defaults)
        self._init_flats()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        first = next(iter(self._all_params()), None)
        if first is None:
            return loss
        steps, _ = self._flats(first.device)
        offset = 0
        for group in self.param_groups:
            for run in self._runs(group, offset, steps):
                self._adamw_run(run, group, group["decoupled"])
            offset += len(group["params"])
        return loss


class FusedLAMB(_FusedAdamBase):
    """LAMB: Adam's direction with a layer-wise trust ratio.

    For every parameter tensor of a group with ``adapt=True``:

        m, v  as FusedAdamW (on g * gs)
        u  = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p
        r  = ||p||_2 / ||u||_2   if both > 0 else 1
        r  = min(r, max_trust)   with trust_clip
        p -= lr * r * u

    Groups with ``adapt=False`` take exactly the ``FusedAdamW`` (decoupled)
    step.  On GPU an adapted group is the tick plus three HIP launches per
    32 tensors (moments and pair square sums, per-tensor ratio, step; u is
    recomputed in the step, no update buffer); no host sync, and the amp
    overflow flag skips all of them on device.  On CPU (and as the oracle)
    the same formula runs in torch with the norms taken in float64.

    ``trust_ratios``: as ``FusedLARS.trust_ratios``.  The state is
    ``FusedAdamW``'s.
    """

    def __init__(self, params, lr: float, betas=(0.9, 0.999),
                 eps: float = 1e-6, weight_decay: float = 0.01,
                 trust_clip: bool = False, max_trust: float = 10.0):
        _check_adam_args(lr, betas, eps, weight_decay)
        if max_trust <= 0.0:
            raise ValueError(f"invalid max_trust {max_trust}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps,
                        weight_decay=weight_decay,
                        trust_clip=bool(trust_clip), max_trust=max_trust,
                        adapt=True)
        super().__init__(params, defaults)
        self._init_flats()
        self.trust_ratios = None
        self._partials = None

    _ratio_buffer = FusedLARS._ratio_buffer

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = self._all_params()
        if not params:
            return loss
        steps, _ = self._flats(params[0].device)
        ratios = self._ratio_buffer(params[0].device, len(params))
        offset = 0
        for group in self.param_groups:
            for run in self._runs(group, offset, steps):
                if group["adapt"]:
                    self._lamb_run(run, group, ratios)
                else:
                    self._adamw_run(run, group, True)
            offset += len(group["params"])
        return loss

    def _lamb_run(self, run, group, ratios):
        start, params, grads, ms, vs = run
        n = len(params)
        lr, (b1, b2) = group["lr"], group["betas"]
        eps, wd = group["eps"], group["weight_decay"]
        trust_clip, max_trust = group["trust_clip"], group["max_trust"]
        steps = self._steps[start:start + n]
        ratios = ratios[start:start + n]
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
            coefs = self._coefs[ADAM_NCOEF * start:ADAM_NCOEF * (start + n)]
            ext.fused_lamb(params, grads, ms, vs, steps, coefs,
                           self._partials, ratios, lr, b1, b2, eps, wd,
                           bool(trust_clip), max_trust,
                           amp_mod.pending_found_inf(),
                           amp_mod.pending_grad_scale())
            # raw-pointer writes don't bump Tensor._version (see FusedSGD)
            clear_weight_cache()
            return
        # reference path: norms in float64, the rest in fp32 torch ops
        steps.add_(1)
        for i, (p, g, m, v, s) in enumerate(zip(params, grads, ms, vs,
                                                steps.tolist())):
            bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
            _moments(g, m, v, b1, b2)
            u = (m / bc1).div_((v / bc2).sqrt_().add_(eps))
            if wd != 0:
                u.add_(p, alpha=wd)
            wn = float(torch.linalg.vector_norm(p.double()))
            un = float(torch.linalg.vector_norm(u.double()))
            r = 1.0
            if wn > 0 and un > 0:
                r = wn / un
                if trust_clip:
                    r = min(r, max_trust)
            ratios[i] = r
            p.add_(u, alpha=-(lr * float(ratios[i])))


def decay_param_groups(model, weight_decay: float = 0.0):
    """Two parameter groups for ``FusedAdamW`` / ``FusedLAMB``: tensors with
    ``ndim <= 1`` (BatchNorm scale and shift, biases) are not decayed and,
    for LAMB, not adapted (``adapt=False``: the AdamW step); the rest get
    ``weight_decay`` and ``adapt=True``.  Every trainable parameter lands in
    exactly one group; within a group the model's parameter order is
    kept."""
    decayed, plain = [], []
    for p in model.parameters():
        if not p.requires_grad:
            continue
        (plain if p.ndim <= 1 else decayed).append(p)
    return [
        dict(params=decayed, adapt=True, weight_decay=weight_decay),
        dict(params=plain, adapt=False, weight_decay=0.0),
    ]


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
