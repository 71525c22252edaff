"""HeightCompression (pcdet/models/backbones_2d/map_to_bev/height_compression.py of the reference): the encoded sparse tensor as a dense BEV
map with the z slices stacked into the channels, channel index c * D + d.  One kernel writes the whole NHWC canvas (no clear pass);
`spatial_features` is the NCHW-shaped view of it, the form PointPillarScatter hands BaseBEVBackbone.

In training mode (behind a VoxelResBackBone8x built with HIP_TRAIN) it records its own backward closure: the canvas gradient BackboneTrain
returns, gathered per row (pcp_spconv_dense_backward).  The sparse stage is fp32: in the bf16 loop the canvas is handed over as bf16, the
dtype BackboneTrain's first layer reads, and the gradient is taken back as float32."""
import torch
import torch.nn as nn

from pcp_amd import ops

from ...packed import train_tape


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg.NUM_BEV_FEATURES

    def forward(self, batch_dict):
        t = batch_dict['encoded_spconv_tensor']
        if self.training:
            return self._forward_train(batch_dict, t)
        canvas = t.dense_nhwc()
        if canvas.shape[3] != self.num_bev_features:
            raise ValueError('HeightCompression: NUM_BEV_FEATURES is %d, the encoded tensor gives %d channels x %d slices'
                             % (self.num_bev_features, t.features.shape[1], t.spatial_shape[0]))
        batch_dict['spatial_features'] = ops.nchw_view(canvas)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        return batch_dict

    def _forward_train(self, batch_dict, t):
        from pcp_amd import train_layers as tl
        from pcp_amd import train_ops as tops
        rows, C = int(t.features.shape[0]), int(t.features.shape[1])
        B, (D, H, W) = t.batch_size, t.spatial_shape
        if C * D != self.num_bev_features:
            raise ValueError('HeightCompression: NUM_BEV_FEATURES is %d, the encoded tensor gives %d channels x %d slices' % (self.num_bev_features, C, D))
        if rows:
            canvas = t.dense_nhwc()
        else:
            canvas = torch.zeros((B, H, W, C * D), dtype=torch.float32, device=t.features.device)
        if tl.mp_mode():
            canvas = canvas.to(torch.bfloat16)

        def backward(g):
            """g: Act, the gradient of the canvas (B, H, W, C * D).  Returns the float32 gradient of the encoded rows (rows, C)."""
            if not rows:
                return torch.zeros((0, C), dtype=torch.float32, device=g.t.device)
            return tops.spconv_dense_backward(tl.as_f32(g.t, g.off, g.c), t.indices, (B, D, H, W), C)
        batch_dict['spatial_features'] = ops.nchw_view(canvas)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        train_tape(batch_dict).append(('map_to_bev', backward))
        return batch_dict
