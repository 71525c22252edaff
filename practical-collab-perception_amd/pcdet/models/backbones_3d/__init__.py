"""3-D backbones: the residual sparse backbone of the SECOND models (inference).  Detector3DTemplate.build_backbone_3d reports a clear error
for a config that names another one."""
from .spconv_backbone import VoxelResBackBone8x

__all__ = {
    'VoxelResBackBone8x': VoxelResBackBone8x,
}
