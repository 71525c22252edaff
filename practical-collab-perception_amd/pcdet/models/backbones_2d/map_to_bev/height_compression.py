"""HeightCompression (pcdet/models/backbones_2d/map_to_bev/height_compression.py of the reference): the encoded sparse tensor as a dense BEV
map with the z slices stacked into the channels, channel index c * D + d.  One kernel writes the whole NHWC canvas (no clear pass);
`spatial_features` is the NCHW-shaped view of it, the form PointPillarScatter hands BaseBEVBackbone."""
import torch.nn as nn

from pcp_amd import ops


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg.NUM_BEV_FEATURES

    def forward(self, batch_dict):
        t = batch_dict['encoded_spconv_tensor']
        canvas = t.dense_nhwc()
        if canvas.shape[3] != self.num_bev_features:
            raise ValueError('HeightCompression: NUM_BEV_FEATURES is %d, the encoded tensor gives %d channels x %d slices'
                             % (self.num_bev_features, t.features.shape[1], t.spatial_shape[0]))
        batch_dict['spatial_features'] = ops.nchw_view(canvas)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        return batch_dict
