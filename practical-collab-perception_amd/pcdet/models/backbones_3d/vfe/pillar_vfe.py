"""PillarVFE on gfx950: the classic PointPillar front end (pcdet/models/backbones_3d/vfe/pillar_vfe.py of the reference) -- hard voxelisation
(spconv's CPU generator, here pcp_hard_voxelize) and ONE PFN layer on the padded (M, T, C) voxel tensor (pcp_pillar_vfe).  Inference only.
Constructor signature, attributes and state_dict keys are the reference's (pfn_layers.0.linear.weight, pfn_layers.0.norm.* or
pfn_layers.0.linear.bias), so a published PointPillar checkpoint loads unchanged.

The voxel tensors come from the loader when it supplies them (`voxels`, `voxel_num_points`, `voxel_coords` as device tensors, the layout of
the reference's collated batch); otherwise the module voxelises batch_dict['points'] itself with the dataset's transform_points_to_voxels
entry (MAX_POINTS_PER_VOXEL, MAX_NUMBER_OF_VOXELS[mode]) and writes the three keys back.
"""
import torch
import torch.nn as nn

from pcp_amd import ops, pack

from .vfe_template import VFETemplate

MAX_PFN_LAYERS = 1


class PFNLayer(nn.Module):
    """Parameter container only (Linear + BatchNorm1d eps 1e-3, or Linear with bias); the arithmetic runs inside k_pillar_vfe."""

    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.part = 50000

    def folded(self):
        w = self.linear.weight.detach()
        if self.use_norm:
            n = self.norm
            return pack.fold_bn(w, n.weight.detach(), n.bias.detach(), n.running_mean, n.running_var, n.eps)
        return w.float(), self.linear.bias.detach().float()


class PillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        self.num_raw_point_features = int(num_point_features)
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = self.model_cfg.NUM_FILTERS
        assert len(self.num_filters) > 0
        if len(self.num_filters) > MAX_PFN_LAYERS:
            raise NotImplementedError('PillarVFE runs %d PFN layer (every stock PointPillar config has NUM_FILTERS: [64]); NUM_FILTERS has %d '
                                      'entries' % (MAX_PFN_LAYERS, len(self.num_filters)))
        out = int(self.num_filters[-1])
        if out % 16 or not 16 <= out <= ops.PILLAR_VFE_MAX_OUT:
            raise NotImplementedError('PillarVFE: NUM_FILTERS[-1] is a multiple of 16 up to %d, got %d' % (ops.PILLAR_VFE_MAX_OUT, out))
        num_filters = [num_point_features] + list(self.num_filters)
        self.pfn_layers = nn.ModuleList([
            PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
            for i in range(len(num_filters) - 1)])
        self.voxel_x = voxel_size[0]
        self.voxel_y = voxel_size[1]
        self.voxel_z = voxel_size[2]
        self.x_offset = self.voxel_x / 2 + point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + point_cloud_range[2]
        # the voxeliser of the `points` path (not in the reference, whose DataProcessor voxelises in the loader)
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        self.grid_size = kwargs.get('grid_size', None)
        vox = kwargs.get('hard_voxel', None) or {}
        self.max_points_per_voxel = vox.get('MAX_POINTS_PER_VOXEL', None)
        self.max_number_of_voxels = vox.get('MAX_NUMBER_OF_VOXELS', None)

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('PillarVFE is inference only: the HIP training path covers DynPillarVFE; call .eval()')
        return super().train(mode)

    def _build_packed(self):
        w, b = self.pfn_layers[0].folded()
        return dict(w=w.contiguous(), b=b.contiguous())

    def voxelize(self, points, batch_size):
        """hard voxelisation of collated rows with the dataset's transform_points_to_voxels entry -> ops.HardVoxelResult"""
        if self.max_points_per_voxel is None or self.max_number_of_voxels is None:
            raise KeyError('PillarVFE got neither voxels nor a transform_points_to_voxels entry (MAX_POINTS_PER_VOXEL, MAX_NUMBER_OF_VOXELS) '
                           'in the dataset\'s DATA_PROCESSOR to voxelise `points` with')
        mv = self.max_number_of_voxels
        if isinstance(mv, dict):
            mv = mv['test']                       # inference only
        if points.dtype != torch.float32 or not points.is_contiguous():
            points = points.float().contiguous()
        if points.shape[1] != 1 + self.num_raw_point_features:
            raise ValueError('PillarVFE voxelises rows of %d columns (frame index + %d point features), got %d'
                             % (1 + self.num_raw_point_features, self.num_raw_point_features, points.shape[1]))
        r = self.point_cloud_range
        grid_size = self.grid_size if self.grid_size is not None else [round((r[3 + i] - r[i]) / self.voxel_size[i]) for i in range(3)]
        grid = ops.make_grid(r, self.voxel_size, grid_size, batch_size)
        return ops.hard_voxelize(points, grid, r[5], int(self.max_points_per_voxel), int(mv))

    def forward(self, batch_dict, **kwargs):
        if self.training:
            raise NotImplementedError('PillarVFE is inference only')
        if batch_dict.get('voxels', None) is None:
            points = batch_dict['points']
            batch_size = batch_dict.get('batch_size', None)
            if batch_size is None:
                batch_size = int(points[:, 0].max().item()) + 1 if points.shape[0] else 1
            res = self.voxelize(points, int(batch_size))
            batch_dict['voxels'], batch_dict['voxel_num_points'], batch_dict['voxel_coords'] = res.voxels, res.voxel_num_points, res.voxel_coords
        voxels, num, coords = batch_dict['voxels'], batch_dict['voxel_num_points'], batch_dict['voxel_coords']
        if not voxels.is_cuda:
            raise RuntimeError('PillarVFE needs CUDA/ROCm tensors; there is no CPU fallback')
        pk = self.packed()
        pf = ops.pillar_vfe(voxels.float().contiguous(), num.int().contiguous(), coords.int().contiguous(),
                            (self.voxel_x, self.voxel_y, self.voxel_z), (self.x_offset, self.y_offset, self.z_offset), pk['w'], pk['b'],
                            use_absolute_xyz=bool(self.use_absolute_xyz), with_distance=bool(self.with_distance))
        batch_dict['pillar_features'] = pf
        return batch_dict
