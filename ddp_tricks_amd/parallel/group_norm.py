"""convert_group_norm — swap the framework's BatchNorm2d modules for
GroupNorm in place: the normalisation for small per-rank batches, with no
cross-rank traffic and no running buffers."""
from __future__ import annotations

import torch.nn as nn

from ..ops.modules import BatchNorm2d, GroupNorm


def _convert_one(bn, num_groups, name):
    if bn.num_features % num_groups:
        raise ValueError(
            f"convert_group_norm: layer '{name}' has {bn.num_features} "
            f"channels, which num_groups={num_groups} does not divide")
    if not bn.affine:
        raise ValueError(f"convert_group_norm: layer '{name}' is not affine")
    gn = GroupNorm(num_groups, bn.num_features, eps=bn.eps,
                   fuse_relu=getattr(bn, "fuse_relu", False))
    # the SAME Parameter objects: optimizers, DDP buckets and checkpoints
    # built before or after the conversion see one set; the running buffers
    # are dropped
    gn._parameters["weight"] = bn._parameters["weight"]
    gn._parameters["bias"] = bn._parameters["bias"]
    gn.training = bn.training
    return gn


def convert_group_norm(module: nn.Module, num_groups: int = 32,
                       _name: str = "") -> nn.Module:
    """Replace every ``ops.modules.BatchNorm2d`` under ``module`` (or
    ``module`` itself) by a ``GroupNorm(num_groups)`` sharing its weight and
    bias Parameters and its ``fuse_relu``; BatchNorm1d layers stay.  A layer
    whose channel count ``num_groups`` does not divide is a ValueError naming
    it.  Returns the converted root."""
    if isinstance(module, BatchNorm2d):
        return _convert_one(module, num_groups, _name)
    for name, child in list(module.named_children()):
        full = f"{_name}.{name}" if _name else name
        new = convert_group_norm(child, num_groups, full)
        if new is not child:
            module._modules[name] = new
    return module
