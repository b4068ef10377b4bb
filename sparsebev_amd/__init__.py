"""sparsebev_amd -- MI355X (gfx950) native implementation of SparseBEV's decoder hot path:
adaptive spatio-temporal sampling + adaptive mixing + scale-adaptive self attention, behind the
reference's own operator / registry interfaces (msmv_sampling, SparseBEVTransformer).

Python here is host glue (tensors, streams, torch.distributed); the work is done by hand-written HIP
kernels in ``csrc/libsbev_hip.so`` bound through a C ABI (``include/sbev_hip.h``).  Importing the
operator modules without the built library raises -- there is no CPU / PyTorch fallback.
"""
from ._lib import load as load_library, SbevError, LIB_PATH   # noqa: F401

__all__ = ['load_library', 'SbevError', 'LIB_PATH', 'SparseBEVHead', 'SparseBEVTrainHead', 'FusedAdamW', 'ImageFrontEnd', 'ImageGeometry', 'FPNNeck',
           'ResNetBackbone', 'SparseBEV']


def __getattr__(name):
    # the heads pull in the whole operator stack: imported on first use
    if name == 'SparseBEVHead':
        from .head import SparseBEVHead
        return SparseBEVHead
    if name == 'SparseBEVTrainHead':
        from .head_train import SparseBEVTrainHead
        return SparseBEVTrainHead
    if name == 'FusedAdamW':
        from .optim import FusedAdamW
        return FusedAdamW
    if name == 'ImageFrontEnd':
        from .image_front import ImageFrontEnd
        return ImageFrontEnd
    if name == 'ImageGeometry':
        from .image_geom import ImageGeometry
        return ImageGeometry
    if name == 'FPNNeck':
        from .fpn import FPNNeck
        return FPNNeck
    if name == 'ResNetBackbone':
        from .resnet import ResNetBackbone
        return ResNetBackbone
    if name == 'SparseBEV':
        from .detector import SparseBEV
        return SparseBEV
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
