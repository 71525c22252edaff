"""VoxelResBackBone8x on gfx950 (pcdet/models/backbones_3d/spconv_backbone.py of the reference): four stages of residual submanifold blocks,
three stride-2 sparse convs between them and the (3, 1, 1) conv that halves z at the end, all on pcp_spconv3d.  Inference only unless the
model config sets MODEL.BACKBONE_3D.HIP_TRAIN (then train() is allowed and a training forward runs second_train_path.VoxelBackboneTrain).  Module nesting
and state_dict keys are the reference's (conv_input.0.weight, conv1.0.conv1.weight / .bias, conv1.0.bn1.*, conv2.0.0.weight, ...,
conv_out.0.weight), so a published SECOND checkpoint loads by name.

Every conv runs with its BatchNorm (and its own bias) folded and its ReLU / residual add in the kernel's epilogue: 21 conv launches per forward.
The submanifold layers of one stage share one neighbour table (`subm1` and `res1` have the same sites); each of the four strided layers
reads its output row count back once.

MODEL.BACKBONE_3D.DEVICE_COUNTS (opt-in, with MODEL.VFE.DEVICE_COUNTS): no read-back.  Every level's row count stays on the device and its
launches and buffers are sized by a capacity: the input's row count for the voxels, the exact bound min(capacity_in * prod(ceil(k / s)),
output sites) for a strided layer, or the entry of the optional ROW_CAPACITY list (level 0 = voxels, 1 .. 4 = spconv2, spconv3, spconv4,
spconv_down2; a null entry keeps the bound).  A level that holds more rows than its ROW_CAPACITY drops its tail and sets a bit of
batch_dict['_pcp_dev_status'], which the forward's final read turns into a RuntimeError.  The buffers belong to the module (one set per model
replica): a forward overwrites the previous forward's sparse tensors.
"""
from functools import partial

import torch.nn as nn

from pcp_amd import spconv

from ...utils.spconv_utils import replace_feature  # noqa: F401  (re-exported as in the reference)
from ..packed import train_tape

INFERENCE_ONLY = 'inference only'


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm', norm_fn=None):
    if conv_type == 'subm':
        conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == 'spconv':
        conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    else:
        raise NotImplementedError('post_act_block: conv_type %r (subm and spconv have kernels)' % (conv_type,))
    return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(spconv.SparseModule):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + x): two launches, the second with the residual add and the ReLU in its epilogue"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        assert norm_fn is not None
        if downsample is not None or stride != 1:
            raise NotImplementedError('SparseBasicBlock: stride 1 without a downsample branch (every block of VoxelResBackBone8x)')
        self.conv1 = spconv.SubMConv3d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=True, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=True, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride
        self._block_packed = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_packed())

    def invalidate_packed(self):
        self._block_packed = None

    def _apply(self, fn, *args, **kwargs):
        self._block_packed = None
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode=True):
        if mode != self.training:
            self._block_packed = None
        return super().train(mode)

    def forward(self, x):
        if self.training:
            raise NotImplementedError(INFERENCE_ONLY)
        if self._block_packed is None:
            self._block_packed = (self.conv1.packed_weight(self.bn1), self.conv2.packed_weight(self.bn2))
        (w1, b1), (w2, b2) = self._block_packed
        out = self.conv1.run(x, w1, b1, relu=True)
        return self.conv2.run(out, w2, b2, residual=x.features, relu=True)


class VoxelResBackBone8x(nn.Module):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        if self.model_cfg.get('NUM_POINT_FEATURES', None) is not None:
            input_channels = self.model_cfg.NUM_POINT_FEATURES
        nx, ny, nz = (int(v) for v in grid_size)
        self.sparse_shape = [nz + 1, ny, nx]                       # grid_size[::-1] + [1, 0, 0]
        block, res = post_act_block, SparseBasicBlock
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        self.conv1 = spconv.SparseSequential(*[res(16, 16, norm_fn=norm_fn, indice_key='res1') for _ in range(2)])
        stages = []
        for i, (cin, cout, pad) in enumerate(((16, 32, 1), (32, 64, 1), (64, 128, (0, 1, 1))), start=2):
            stages.append(spconv.SparseSequential(
                block(cin, cout, 3, norm_fn=norm_fn, stride=2, padding=pad, indice_key='spconv%d' % i, conv_type='spconv'),
                res(cout, cout, norm_fn=norm_fn, indice_key='res%d' % i), res(cout, cout, norm_fn=norm_fn, indice_key='res%d' % i)))
        self.conv2, self.conv3, self.conv4 = stages
        last_pad = self.model_cfg.get('last_pad', 0)
        self.conv_out = spconv.SparseSequential(
            spconv.SparseConv3d(128, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key='spconv_down2'),
            norm_fn(128), nn.ReLU())
        self.num_point_features = 128
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 128}
        self.hip_train = bool(self.model_cfg.get('HIP_TRAIN', False))         # opt-in: the HIP training path (second_train_path.py)
        self._pcp_train = None
        self.device_counts = bool(self.model_cfg.get('DEVICE_COUNTS', False))
        cap = self.model_cfg.get('ROW_CAPACITY', None)
        self.row_capacity = None if cap is None else [None if v is None else int(v) for v in cap]
        if self.device_counts and self.hip_train:
            raise NotImplementedError('MODEL.BACKBONE_3D: DEVICE_COUNTS is an inference form; it cannot be combined with HIP_TRAIN')
        if self.row_capacity is not None and not self.device_counts:
            raise ValueError('MODEL.BACKBONE_3D.ROW_CAPACITY belongs to DEVICE_COUNTS True')
        if self.row_capacity is not None and (len(self.row_capacity) != 5 or any(v is not None and v < 1 for v in self.row_capacity)):
            raise ValueError('MODEL.BACKBONE_3D.ROW_CAPACITY: five entries (voxels, spconv2, spconv3, spconv4, spconv_down2), each null or >= 1')
        self._dev_bufs = spconv.ops.DevBuffers()

    def train(self, mode=True):
        if mode and not self.hip_train:
            raise NotImplementedError(INFERENCE_ONLY)
        return super().train(mode)

    def _forward_train(self, batch_dict):
        from ..second_train_path import VoxelBackboneTrain
        if self._pcp_train is None:
            self._pcp_train = VoxelBackboneTrain(self)
        out, scales = self._pcp_train.forward(batch_dict['voxel_features'], batch_dict['voxel_coords'], batch_dict['batch_size'],
                                              trusted=batch_dict.get('_pcp_voxels_trusted', False))
        batch_dict.update({
            'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8,
            'multi_scale_3d_features': dict(zip(('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'), scales)),
            'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}})
        train_tape(batch_dict).append(('backbone_3d', self._pcp_train.backward))
        return batch_dict

    def forward(self, batch_dict):
        if self.training:
            if not self.hip_train:
                raise NotImplementedError(INFERENCE_ONLY)
            return self._forward_train(batch_dict)
        feats, coords = batch_dict['voxel_features'], batch_dict['voxel_coords']
        if not feats.is_cuda:
            raise RuntimeError('VoxelResBackBone8x needs CUDA/ROCm tensors; there is no CPU fallback')
        x = spconv.SparseConvTensor(features=feats.float().contiguous(), indices=coords.int().contiguous(), spatial_shape=self.sparse_shape,
                                    batch_size=batch_dict['batch_size'])
        x.trusted_indices = bool(batch_dict.get('_pcp_voxels_trusted', False))
        dev = None
        if self.device_counts:
            if batch_dict.get('_pcp_voxel_count', None) is None or not x.trusted_indices:
                raise RuntimeError('VoxelResBackBone8x with DEVICE_COUNTS needs the voxels of a DynMeanVFE built with DEVICE_COUNTS '
                                   '(a device-side count, distinct sites inside the grid)')
            dev = spconv.DeviceCounts(batch_dict['_pcp_dev_status'], self._dev_bufs, self.row_capacity, input_capacity=int(coords.shape[0]))
            if dev.capacity_of(0) is not None and dev.capacity_of(0) < int(coords.shape[0]):
                raise RuntimeError('sparse backbone: %d voxel rows exceed ROW_CAPACITY[0] = %d' % (int(coords.shape[0]), dev.capacity_of(0)))
            x.with_device_count(batch_dict['_pcp_voxel_count'], dev)
            batch_dict['_pcp_dev_levels'] = dev.levels
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        out = self.conv_out(x_conv4)
        batch_dict.update({
            'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8,
            'multi_scale_3d_features': {'x_conv1': x_conv1, 'x_conv2': x_conv2, 'x_conv3': x_conv3, 'x_conv4': x_conv4},
            'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}})
        return batch_dict
