"""DynMeanVFE on gfx950 (pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py of the reference): the mean of every point column per voxel of the 3D
grid, voxels in ascending merged id (what torch.unique returns), on pcp_mean_vfe -- no sort, no float atomics.  No parameters.  Inference only
unless the model config sets MODEL.VFE.HIP_TRAIN: then train() is allowed, the forward is the same and its backward closure returns None (the
points carry no gradient).

MODEL.VFE.DEVICE_COUNTS (opt-in, with MODEL.BACKBONE_3D.DEVICE_COUNTS): the forward reads nothing back.  `voxel_features` / `voxel_coords` then
hold max(N, 1) rows, the voxel count stays on the device (batch_dict['_pcp_voxel_count']) and the error word (frames out of order) travels in
batch_dict['_pcp_dev_status'] to the forward's final read, which raises the same ValueError.  The buffers belong to the module (one set per
model replica) and are overwritten by its next forward."""
import torch

from pcp_amd import ops

from ...packed import train_tape
from .vfe_template import VFETemplate


class DynamicMeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = int(num_point_features)
        if self.model_cfg.get('NUM_POINT_FEATURES', None) is not None:
            self.num_raw_point_features = int(self.model_cfg.NUM_POINT_FEATURES)
        else:
            self.num_raw_point_features = self.num_point_features
        self.grid_size = [int(v) for v in grid_size]
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self._workspace = None
        self.hip_train = bool(self.model_cfg.get('HIP_TRAIN', False))
        self.device_counts = bool(self.model_cfg.get('DEVICE_COUNTS', False))
        if self.device_counts and self.hip_train:
            raise NotImplementedError('MODEL.VFE: DEVICE_COUNTS is an inference form; it cannot be combined with HIP_TRAIN')
        self._dev_bufs = ops.DevBuffers()

    def get_output_feature_dim(self):
        return self.num_raw_point_features

    def train(self, mode=True):
        if mode and not self.hip_train:
            raise NotImplementedError('inference only')
        return super().train(mode)

    def _build_packed(self):
        return {}

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        if self.training and not self.hip_train:
            raise NotImplementedError('inference only')
        points = batch_dict['points']
        if not points.is_cuda:
            raise RuntimeError('DynMeanVFE needs CUDA/ROCm tensors; there is no CPU fallback')
        if points.dtype != torch.float32 or not points.is_contiguous():
            points = points.float().contiguous()
        batch_size = batch_dict.get('batch_size', None)
        if batch_size is None:
            batch_size = int(points[:, 0].max().item()) + 1 if points.shape[0] else 1
            batch_dict['batch_size'] = batch_size
        grid = ops.make_grid(self.point_cloud_range, self.voxel_size, self.grid_size, int(batch_size))
        if self.device_counts:
            feats, coords, status = ops.mean_vfe_dev(points, grid, self.num_raw_point_features, nz=self.grid_size[2], bufs=self._dev_bufs)
            batch_dict.update({'voxel_features': feats, 'voxel_coords': coords, '_pcp_voxels_trusted': True, '_pcp_voxel_count': status[0:1],
                               '_pcp_dev_status': status})
            return batch_dict
        feats, coords, _ = ops.mean_vfe(points, grid, self.num_raw_point_features, nz=self.grid_size[2], workspace=self._workspace)
        batch_dict['voxel_features'] = feats
        batch_dict['voxel_coords'] = coords
        batch_dict['_pcp_voxels_trusted'] = True          # distinct sites inside the grid: the backbone need not read a count back to check
        if self.training:
            train_tape(batch_dict).append(('vfe', lambda g: None))
        return batch_dict
