from .ddp import DistributedDataParallel  # noqa: F401
from .group_norm import convert_group_norm  # noqa: F401
from .sync_bn import (  # noqa: F401
    convert_sync_batchnorm, convert_syncbn_model,
)
