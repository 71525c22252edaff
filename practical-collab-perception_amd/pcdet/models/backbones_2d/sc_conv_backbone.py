"""SCConvBackbone2dStride4 / SCConvBackbone2dStride1 on gfx950 (reference: workspace/sc_conv.py:14-208), the 2-D backbones of the
nuScenes PointPillar-Jr models.

Same parameter tree as the reference (stem.{0..3}, main_pass.{0..6}, conv_skip.{0,1}, conv_out.{0,1}; inside a bottleneck conv1_a / bn1_a,
conv1_b / bn1_b, k1.{0,1}, scconv.k2.{1,2} / k3.{0,1} / k4.{0,1}, conv3 / bn3), so checkpoints load unchanged.  Inference forward of one
SCBottleneck on NHWC buffers, BatchNorm folded into every conv:
  conv1_a | conv1_b + ReLU       -> ONE 1x1 launch with 2 * group_width outputs: [a | b]
  k1 + ReLU                      -> 3x3 conv on the a window, written into window 0 of the cat buffer conv3 reads
  k2 = AvgPool2d(4) -> 3x3       -> pcp_avgpool_nhwc on the b window, then a 3x3 conv at the pooled size (no ReLU)
  k3                             -> 3x3 conv on the b window (no ReLU)
  k3 * sigmoid(b + up(k2))       -> pcp_sc_gate, in place over the k3 output
  k4 + ReLU                      -> 3x3 conv, written into window 1 of the cat buffer
  relu(conv3(cat) + x)           -> 1x1 launch with the residual added before the activation
The ConvTranspose of main_pass and conv_skip write the two windows of conv_out's input: there is no torch.cat anywhere.

train() mode (GPU only): pcdet/models/train_path.py SCBackboneTrain runs the same graph layer by layer with batch-statistics BatchNorm
(ConvBNAct: conv1_a and conv1_b stay two layers, each with its own BatchNorm, writing the two windows of [a | b]), keeps the un-gated k3
output, and records its backward on the tape: pcp_add_relu_backward, the conv / BatchNorm gradients, pcp_sc_gate_backward and
pcp_avgpool_nhwc_backward, with every gradient fan-in added in a fixed order (no atomics: a step repeats bit for bit).
"""
from functools import partial

import torch
import torch.nn as nn

from pcp_amd import lib, ops, pack

from ..convnet import PackedConv, _fold, pack_conv_module
from ..packed import PackedModule, train_tape

POOLING_R = 4          # SCBottleneck.pooling_r


class SCConv(nn.Module):
    """parameter container (reference :14-44); k2.0 is the AvgPool2d"""

    def __init__(self, inplanes, planes, norm_layer):
        super().__init__()
        self.k2 = nn.Sequential(nn.AvgPool2d(kernel_size=POOLING_R, stride=POOLING_R),
                                nn.Conv2d(inplanes, planes, 3, stride=1, padding=1, bias=False), norm_layer(planes))
        self.k3 = nn.Sequential(nn.Conv2d(inplanes, planes, 3, stride=1, padding=1, bias=False), norm_layer(planes))
        self.k4 = nn.Sequential(nn.Conv2d(inplanes, planes, 3, stride=1, padding=1, bias=False), norm_layer(planes))


class SCBottleneck(nn.Module):
    """parameter container (reference :47-119) for the only form the backbones use: stride 1, no avd, no downsample, cardinality 1,
    group_width = planes / 2"""

    def __init__(self, inplanes, planes, norm_layer):
        super().__init__()
        gw = int(planes * (32 / 64.))
        self.conv1_a = nn.Conv2d(inplanes, gw, kernel_size=1, bias=False)
        self.bn1_a = norm_layer(gw)
        self.conv1_b = nn.Conv2d(inplanes, gw, kernel_size=1, bias=False)
        self.bn1_b = norm_layer(gw)
        self.k1 = nn.Sequential(nn.Conv2d(gw, gw, 3, stride=1, padding=1, bias=False), norm_layer(gw))
        self.scconv = SCConv(gw, gw, norm_layer)
        self.conv3 = nn.Conv2d(gw * 2, planes, kernel_size=1, bias=False)
        self.bn3 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)


def conv_bn_relu(cin, cout, kernel_size=3, stride=1, padding=0, norm_layer=nn.BatchNorm2d):
    """reference :122-127.  The default norm_layer is nn.BatchNorm2d (eps 1e-5): conv_out keeps it, every other layer passes eps 1e-3"""
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False), norm_layer(cout),
                         nn.ReLU(inplace=True))


class _PackedBottleneck:
    """the launches of one SCBottleneck (module docstring)"""

    def __init__(self, blk):
        self.gw = blk.conv1_a.out_channels
        self.planes = blk.conv3.out_channels
        wa, ba = _fold(blk.conv1_a, blk.bn1_a, out_axis=0)
        wb, bb = _fold(blk.conv1_b, blk.bn1_b, out_axis=0)
        self.conv1 = PackedConv('plain', blk.conv1_a.in_channels, 2 * self.gw, True, pack.pack_plain(torch.cat([wa, wb], 0), torch.cat([ba, bb], 0)))
        self.k1 = pack_conv_module(blk.k1[0], blk.k1[1], relu=True)
        self.k2 = pack_conv_module(blk.scconv.k2[1], blk.scconv.k2[2], relu=False)
        self.k3 = pack_conv_module(blk.scconv.k3[0], blk.scconv.k3[1], relu=False)
        self.k4 = pack_conv_module(blk.scconv.k4[0], blk.scconv.k4[1], relu=True)
        self.conv3 = pack_conv_module(blk.conv3, blk.bn3, relu=True)

    def run(self, x):
        gw = self.gw
        B, H, W, _ = x.shape
        ab = self.conv1.run(x)                                                      # (B, H, W, 2 gw) = [a | b]
        cat = torch.empty((B, H, W, 2 * gw), dtype=torch.float32, device=x.device)
        self.k1.run(ab, out=cat, in_ch_off=0, out_ch_off=0)
        pooled = ops.avgpool_nhwc(ab, POOLING_R, in_ch_off=gw, c=gw)
        s = self.k2.run(pooled)
        t = self.k3.run(ab, in_ch_off=gw)
        ops.sc_gate(t, ab, s, gw, x_ch_off=gw)                                      # in place: t = t * sigmoid(b + up(s))
        self.k4.run(t, out=cat, out_ch_off=gw)
        c3 = self.conv3
        return ops.pointwise(cat, c3.w, c3.b, lib.PW_PLAIN, c3.cin, c3.cout, c3.cout_pad, relu=True, residual=x,
                             residual_before_relu=True)


class _SCBackboneBase(PackedModule):
    """shared forward of the two backbones: stem -> (conv_skip | main_pass) -> conv_out"""

    def _build_packed(self):
        def seq_convs(seq):
            return pack_conv_module(seq[0], seq[1], relu=True)
        mp = list(self.main_pass)
        return dict(stem0=seq_convs(self.stem[0]), stem_blocks=[_PackedBottleneck(b) for b in list(self.stem)[1:]],
                    skip=seq_convs(self.conv_skip), main0=seq_convs(mp[0]), main_blocks=[_PackedBottleneck(b) for b in mp[1:4]],
                    up=pack_conv_module(mp[4], mp[5], relu=True), out=seq_convs(self.conv_out))

    def _forward_train(self, data_dict):
        from pcp_amd.train_layers import Act
        from ..train_path import SCBackboneTrain
        if getattr(self, '_pcp_train', None) is None:
            self._pcp_train = SCBackboneTrain(self)
        self._pcp_train.check_input(data_dict['spatial_features'])          # NotImplementedError / ValueError before any launch
        self.invalidate_packed()
        out = self._pcp_train.forward(Act(ops.as_nhwc(data_dict['spatial_features'])))
        data_dict['spatial_features_2d'] = ops.nchw_view(out.t)
        train_tape(data_dict).append(('backbone_2d', self._pcp_train.backward))
        return data_dict

    def forward(self, data_dict):
        if data_dict['spatial_features'] is None:
            raise RuntimeError('%s needs the dense canvas: the VFE skipped it (sparse_first_layer); unset sparse_first_layer'
                               % type(self).__name__)
        if self.training:
            return self._forward_train(data_dict)
        pk = self.packed()
        x = ops.as_nhwc(data_dict['spatial_features'])
        x = pk['stem0'].run(x)
        for blk in pk['stem_blocks']:
            x = blk.run(x)
        B, H, W, _ = x.shape
        main_ch = pk['skip'].cout
        merged = torch.empty((B, H, W, pk['up'].cout + main_ch), dtype=torch.float32, device=x.device)
        pk['skip'].run(x, out=merged, out_ch_off=pk['up'].cout)                    # cat([main, skip]): skip is window 1
        y = pk['main0'].run(x)
        for blk in pk['main_blocks']:
            y = blk.run(y)
        if 2 * y.shape[1] != H or 2 * y.shape[2] != W:
            raise ValueError('%s: the up-sampled main pass (%dx%d) does not match the stem map (%dx%d); the grid needs even stem sizes'
                             % (type(self).__name__, 2 * y.shape[1], 2 * y.shape[2], H, W))
        pk['up'].run(y, out=merged, out_ch_off=0)
        out = pk['out'].run(merged)
        data_dict['spatial_features_2d'] = ops.nchw_view(out)
        return data_dict


class SCConvBackbone2dStride1(_SCBackboneBase):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        self.cfg = model_cfg
        norm_layer = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        stem_ch = model_cfg.STEM_CHANNELS
        self.stem = nn.Sequential(conv_bn_relu(input_channels, stem_ch, kernel_size=3, padding=1, norm_layer=norm_layer),
                                  *[SCBottleneck(stem_ch, stem_ch, norm_layer) for _ in range(3)])
        self.conv_skip = conv_bn_relu(stem_ch, input_channels, kernel_size=1, norm_layer=norm_layer)
        self.main_pass = nn.Sequential(conv_bn_relu(stem_ch, input_channels, kernel_size=3, stride=2, padding=1, norm_layer=norm_layer),
                                       *[SCBottleneck(input_channels, input_channels, norm_layer) for _ in range(3)],
                                       nn.ConvTranspose2d(input_channels, input_channels, kernel_size=2, stride=2, bias=False),
                                       norm_layer(input_channels), nn.ReLU(inplace=True))
        self.conv_out = conv_bn_relu(2 * input_channels, model_cfg.NUM_BEV_FEATURES, kernel_size=3, padding=1)
        self.num_bev_features = model_cfg.NUM_BEV_FEATURES


class SCConvBackbone2dStride4(_SCBackboneBase):
    def __init__(self, model_cfg, input_channels=64):
        super().__init__()
        self.model_cfg = model_cfg
        self.cfg = model_cfg
        norm_layer = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        stem_ch = input_channels * 2
        self.stem = nn.Sequential(conv_bn_relu(input_channels, stem_ch, kernel_size=3, padding=1, stride=2, norm_layer=norm_layer),
                                  *[SCBottleneck(stem_ch, stem_ch, norm_layer) for _ in range(3)])
        main_ch = stem_ch * 2
        self.main_pass = nn.Sequential(conv_bn_relu(stem_ch, main_ch, kernel_size=3, stride=2, padding=1, norm_layer=norm_layer),
                                       *[SCBottleneck(main_ch, main_ch, norm_layer) for _ in range(3)],
                                       nn.ConvTranspose2d(main_ch, main_ch, kernel_size=2, stride=2, bias=False),
                                       norm_layer(main_ch), nn.ReLU(inplace=True))
        self.conv_skip = conv_bn_relu(stem_ch, main_ch, kernel_size=1, norm_layer=norm_layer)
        self.conv_out = conv_bn_relu(2 * main_ch, model_cfg.NUM_BEV_FEATURES, kernel_size=3, padding=1, stride=2)
        self.num_bev_features = model_cfg.NUM_BEV_FEATURES
