from .ddp import DistributedDataParallel  # noqa: F401
from .sync_bn import (  # noqa: F401
    convert_sync_batchnorm, convert_syncbn_model,
)
