from .base_bev_backbone import BaseBEVBackbone
from .sc_conv_backbone import SCConvBackbone2dStride1, SCConvBackbone2dStride4

# registry name -> class (reference: pcdet/models/backbones_2d/__init__.py:1-9; the two SC backbones the reference imports from
# workspace/sc_conv.py are restated in sc_conv_backbone.py, without that module's lovely_tensors import)
__all__ = {
    'BaseBEVBackbone': BaseBEVBackbone,
    'SCConvBackbone2dStride1': SCConvBackbone2dStride1,
    'SCConvBackbone2dStride4': SCConvBackbone2dStride4,
}
