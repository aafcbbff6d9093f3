"""Hand-written gfx950 HIP kernels (``fluxmpi_amd._C``) and their Python wrappers."""
from . import _ext, multi_tensor, optim  # noqa: F401
from .syncbn import SyncBatchNorm2d, convert_sync_batchnorm, sync_batch_norm  # noqa: F401,E402
