"""convert_sync_batchnorm — swap the framework's BatchNorm modules for
SyncBatchNorm in place (the counterpart of apex.parallel's
``convert_syncbn_model`` / ``nn.SyncBatchNorm.convert_sync_batchnorm``)."""
from __future__ import annotations

import torch.nn as nn

from ..ops.modules import BatchNorm1d, BatchNorm2d, SyncBatchNorm


def _convert_one(bn, process_group):
    sync = SyncBatchNorm(bn.num_features, eps=bn.eps, momentum=bn.momentum,
                         affine=bn.affine,
                         track_running_stats=bn.track_running_stats,
                         fuse_relu=getattr(bn, "fuse_relu", False),
                         process_group=process_group)
    # the SAME Parameter / buffer objects: optimizers, DDP buckets and
    # checkpoints built before or after the conversion see one set
    for name, p in bn._parameters.items():
        sync._parameters[name] = p
    for name, b in bn._buffers.items():
        sync._buffers[name] = b
    sync.training = bn.training
    return sync


def convert_sync_batchnorm(module: nn.Module, process_group=None) -> nn.Module:
    """Replace every ``ops.modules.BatchNorm1d/2d`` under ``module`` (or
    ``module`` itself) by a ``SyncBatchNorm`` sharing its parameters,
    buffers and ``fuse_relu``; state_dict keys are unchanged.  Returns the
    converted root."""
    if isinstance(module, (BatchNorm1d, BatchNorm2d)):
        return _convert_one(module, process_group)
    for name, child in list(module.named_children()):
        new = convert_sync_batchnorm(child, process_group)
        if new is not child:
            module._modules[name] = new
    return module


convert_syncbn_model = convert_sync_batchnorm   # apex name parity
