"""World augmentation of a collated training batch on the device (csrc/augment.hip).

The reference augments every sample in its DataLoader workers (pcdet/datasets/augmentor/data_augmentor.py, augmentor_utils.py: numpy and
torch-CPU) and masks the points outside the range afterwards (data_processor.py mask_points_and_boxes_outside_range).  Here the batch
is collated and on the GPU already, so DeviceWorldAugmentor

  * parses DATA_AUGMENTOR the way DataAugmentor.__init__ does and keeps the four world transforms in list order (random_world_flip,
    random_world_rotation, random_world_scaling, random_world_translation); gt_sampling runs in front of them when a DeviceGtSampler is given
    (pcp_amd/gt_sampler.py: it holds the database); every other entry (the local augmentations and dropouts need RoI data, ...) is
    skipped with one logged line;
  * draw(): draws, frame by frame, exactly the numpy calls the reference makes for consecutive samples;
  * apply(): two launches on the current stream (points; gt_boxes + instances_tf) and the float64 se3_from_ego update on the host.

There is no CPU path: apply() needs CUDA tensors.
"""
import ctypes
import logging
import math

import numpy as np
import torch

from . import lib as _lib
from .lib import check
from .ops import _need_cuda, _p, _stream

WORLD_TRANSFORMS = ('random_world_flip', 'random_world_rotation', 'random_world_scaling', 'random_world_translation')
RANGE_FILTER = 'mask_points_and_boxes_outside_range'
GT_SAMPLING = 'gt_sampling'
BOX_WIDTHS = (8, 10)                 # [x y z dx dy dz heading class] / [.. heading vx vy class]
TF_ROWS = (3, 4)                     # instances_tf (B, M, S, 3 | 4, 4)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def rotation_cos_sin(noise_rot):
    """the float32 (cos, sin) of the rotation matrix the reference builds: common_utils.rotate_points_along_z casts the float64 angle to
    float32 (check_numpy_to_torch) and calls torch.cos / torch.sin on it.  The same two torch calls here, so the kernels get the
    reference's bits and evaluate no sine or cosine for the matrix themselves."""
    ang = torch.from_numpy(np.asarray(noise_rot, dtype=np.float64).reshape(-1)).float()
    return torch.cos(ang).numpy(), torch.sin(ang).numpy()


def stage_matrix(stage, p, b):
    """the float64 4x4 of one stage for frame b, or None when the stage leaves the frame alone (a flip that was not drawn)"""
    T = np.eye(4)
    if stage == _lib.AUG_FLIP_X:
        if not p['flip_x'][b]:
            return None
        T[1, 1] = -1.0
    elif stage == _lib.AUG_FLIP_Y:
        if not p['flip_y'][b]:
            return None
        T[0, 0] = -1.0
    elif stage == _lib.AUG_ROTATE:
        c, s = math.cos(float(p['noise_rot'][b])), math.sin(float(p['noise_rot'][b]))
        T[:2, :2] = [[c, -s], [s, c]]
    elif stage == _lib.AUG_SCALE:
        T[0, 0] = T[1, 1] = T[2, 2] = float(p['noise_scale'][b])
    elif stage == _lib.AUG_TRANSLATE:
        T[:3, 3] = p['noise_translate'][b]
    return T


def augment_se3_from_ego(se3_from_ego, stages, p, b):
    """DiscoNet's agent poses under the flips and the rotation: inv(T @ inv(se3)) per stage, as augmentor_utils.py writes it (the
    reference's scaling and translation leave the poses alone).  float64 on the host: a handful of 4x4 per frame."""
    out = {}
    for k, tf in se3_from_ego.items():
        tf = np.asarray(tf, dtype=np.float64)
        for st in stages:
            if st not in (_lib.AUG_FLIP_X, _lib.AUG_FLIP_Y, _lib.AUG_ROTATE):
                continue
            T = stage_matrix(st, p, b)
            if T is not None:
                tf = np.linalg.inv(T @ np.linalg.inv(tf))
        out[k] = tf
    return out


class DeviceWorldAugmentor:
    """aug_cfg: the DATA_AUGMENTOR section (AUG_CONFIG_LIST, DISABLE_AUG_LIST) or the bare list; layout: the dataset layout
    (pcdet.datasets: 'nusc_map' rows carry the HD-map lane direction); data_processor: the DATA_PROCESSOR list -- the range filter runs
    when it names mask_points_and_boxes_outside_range (REMOVE_OUTSIDE_BOXES is not read: the models' own pcp_filter_gt_boxes covers
    the boxes); gt_sampler: a DeviceGtSampler, without one a gt_sampling entry is skipped like the other entries the device path lacks."""

    def __init__(self, aug_cfg, point_cloud_range, layout='car', data_processor=None, logger=None, seed=None, gt_sampler=None):
        self.logger = logger or logging.getLogger(__name__)
        self.rng = np.random.RandomState(seed)          # the generator __call__ draws from (tools/train.py seeds it per rank)
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        assert len(self.point_cloud_range) == 6
        self.layout = layout
        self.hd_map = layout == 'nusc_map'
        self.filter = any(_get(p, 'NAME') == RANGE_FILTER for p in (data_processor or []))
        is_list = isinstance(aug_cfg, (list, tuple))
        cfg_list = aug_cfg if is_list else _get(aug_cfg, 'AUG_CONFIG_LIST', [])
        disabled = [] if is_list else list(_get(aug_cfg, 'DISABLE_AUG_LIST', []) or [])
        self.queue = []                    # (name, config) in list order
        self.skipped = []
        self.gt_sampler = None             # set when the list holds an enabled gt_sampling entry and a sampler was given
        for cur in cfg_list:
            name = _get(cur, 'NAME')
            if name in disabled:
                continue
            if name == GT_SAMPLING and gt_sampler is not None:
                self.gt_sampler = gt_sampler
                self.queue.append((name, cur))
                continue
            if name not in WORLD_TRANSFORMS:
                self.skipped.append(name)
                self.logger.info('DeviceWorldAugmentor: %s is not a world transform of the device path, skipped' % name)
                continue
            self.queue.append((name, cur))
        self.stages = []                   # PCP_AUG_* in the order the kernels apply them
        for name, cur in self.queue:
            if name == GT_SAMPLING:
                continue
            if name == 'random_world_flip':
                for axis in _get(cur, 'ALONG_AXIS_LIST'):
                    assert axis in ('x', 'y'), axis
                    self.stages.append(_lib.AUG_FLIP_X if axis == 'x' else _lib.AUG_FLIP_Y)
            else:
                self.stages.append({'random_world_rotation': _lib.AUG_ROTATE, 'random_world_scaling': _lib.AUG_SCALE,
                                    'random_world_translation': _lib.AUG_TRANSLATE}[name])
        if len(self.stages) > _lib.AUG_MAX_STAGES:
            raise ValueError('%d augmentation stages: the kernels take %d' % (len(self.stages), _lib.AUG_MAX_STAGES))

    @classmethod
    def from_dataset_cfg(cls, dataset_cfg, layout='car', logger=None, seed=None, gt_sampler=None):
        return cls(dataset_cfg.DATA_AUGMENTOR, dataset_cfg.POINT_CLOUD_RANGE, layout, data_processor=_get(dataset_cfg, 'DATA_PROCESSOR', []),
                   logger=logger, seed=seed, gt_sampler=gt_sampler)

    @staticmethod
    def rot_range(cur):
        r = _get(cur, 'WORLD_ROT_ANGLE')
        return [-r, r] if not isinstance(r, (list, tuple)) else list(r)

    def draw(self, batch_size, rng, gt_classes=None):
        """rng: numpy.random.RandomState.  Frame after frame, the calls the reference makes on numpy's global generator for consecutive
        samples, in its order; with RandomState(s) the parameters equal the reference's after np.random.seed(s).  With a gt sampler,
        gt_classes[b] are the class ids of frame b's original boxes and the sampler's draws for frame b come before its world draws."""
        B = int(batch_size)
        if self.gt_sampler is not None and (gt_classes is None or len(gt_classes) != B):
            raise ValueError('draw() with a gt sampler needs gt_classes, the class ids of the original boxes of each of the %d frames' % B)
        p = {'flip_x': np.zeros(B, dtype=bool), 'flip_y': np.zeros(B, dtype=bool), 'noise_rot': np.zeros(B, dtype=np.float64),
             'noise_scale': np.ones(B, dtype=np.float64), 'noise_translate': np.zeros((B, 3), dtype=np.float32)}
        if self.gt_sampler is not None:
            p['gt_sampled'] = []
        for b in range(B):
            if self.gt_sampler is not None:
                p['gt_sampled'].append(self.gt_sampler.draw(gt_classes[b], rng))
            for name, cur in self.queue:
                if name == GT_SAMPLING:
                    continue
                if name == 'random_world_flip':
                    for axis in _get(cur, 'ALONG_AXIS_LIST'):
                        p['flip_%s' % axis][b] = rng.choice([False, True], replace=False, p=[0.5, 0.5])
                elif name == 'random_world_rotation':
                    lo, hi = self.rot_range(cur)
                    p['noise_rot'][b] = rng.uniform(lo, hi)
                elif name == 'random_world_scaling':
                    lo, hi = _get(cur, 'WORLD_SCALE_RANGE')
                    p['noise_scale'][b] = rng.uniform(lo, hi)
                else:
                    std = _get(cur, 'NOISE_TRANSLATE_STD')
                    assert len(std) == 3
                    p['noise_translate'][b] = np.array([rng.normal(0, std[0], 1), rng.normal(0, std[1], 1), rng.normal(0, std[2], 1)],
                                                       dtype=np.float32).T
        return p

    def table(self, p):
        """(B, AUG_TABLE_STRIDE) float32: the per-frame parameters as the kernels read them (include/pcp_hip_train.h)"""
        B = len(p['flip_x'])
        t = np.zeros((B, _lib.AUG_TABLE_STRIDE), dtype=np.float32)
        t[:, 0], t[:, 1] = p['flip_x'], p['flip_y']
        t[:, 2], t[:, 3] = rotation_cos_sin(p['noise_rot'])
        t[:, 4] = np.asarray(p['noise_rot'], dtype=np.float64).astype(np.float32)
        t[:, 5] = np.asarray(p['noise_scale'], dtype=np.float64).astype(np.float32)
        t[:, 6:9] = p['noise_translate']
        return t

    def descriptor(self, batch_size, stages=None, filter=None):
        stages = self.stages if stages is None else list(stages)
        a = _lib.WorldAug()
        a.n_stages = len(stages)
        for i, s in enumerate(stages):
            a.stage[i] = int(s)
        a.batch = int(batch_size)
        a.hd_map = int(self.hd_map)
        a.filter = int(self.filter if filter is None else filter)
        for i, v in enumerate(self.point_cloud_range):
            a.range[i] = v
        return a

    # ---- the two launches ---------------------------------------------------------------------------------------------------------
    def augment_points(self, points, table_dev, batch_size, stages=None, filter=None):
        """points (N, 1 + C) float32 CUDA -> (rows, per-frame kept counts as a numpy array or None).  Filter on: a new tensor holding the
        kept rows in input order (one host read of 4 B bytes); filter off: a new tensor of all N rows, nothing read back."""
        _need_cuda(points, table_dev)
        if points.dim() != 2 or not _lib.AUG_MIN_ROW_STRIDE <= points.shape[1] <= _lib.AUG_MAX_ROW_STRIDE:
            raise ValueError('points of shape %s: the augmentation kernel takes (N, 1 + C) rows of %d (frame index, x y z) up to %d columns'
                             % (tuple(points.shape), _lib.AUG_MIN_ROW_STRIDE, _lib.AUG_MAX_ROW_STRIDE))
        if points.dtype != torch.float32:
            raise ValueError('points are %s: the augmentation kernel reads float32 rows' % points.dtype)
        if self.hd_map and points.shape[1] != 13:
            raise ValueError('HD-map rows have 1 + 12 columns, got %d' % points.shape[1])
        if not 0 < batch_size <= _lib.AUG_MAX_BATCH:
            raise ValueError('batch of %d frames: the augmentation kernels take 1 to %d' % (batch_size, _lib.AUG_MAX_BATCH))
        a = self.descriptor(batch_size, stages, filter)
        L = _lib.load()
        points = points.contiguous()
        if points.data_ptr() % 16:
            points = points.clone()
        n, stride = int(points.shape[0]), int(points.shape[1])
        out = torch.empty_like(points)
        counts = ws = None
        ws_bytes = 0
        if a.filter:
            ws_bytes = int(L.pcp_world_augment_points_workspace_bytes(n))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=points.device)
            counts = torch.empty(batch_size, dtype=torch.int32, device=points.device)
        check(L.pcp_world_augment_points(ctypes.byref(a), _p(table_dev), _p(points), n, stride, _p(out), _p(counts), _p(ws), ws_bytes, _stream()),
              'pcp_world_augment_points')
        if not a.filter:
            return out, None
        kept = counts.cpu().numpy()
        return out[:int(kept.sum())], kept

    def augment_boxes(self, gt_boxes, instances_tf, table_dev, stages=None):
        """gt_boxes (B, M, 8 | 10), instances_tf (B, M, S, 3 | 4, 4) or None -> new tensors; one launch"""
        _need_cuda(gt_boxes, instances_tf, table_dev)
        if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in BOX_WIDTHS:
            raise ValueError('gt_boxes of shape %s: the augmentation kernel takes (B, M, W) with W in %s (x y z dx dy dz heading [vx vy] class)'
                             % (tuple(gt_boxes.shape), BOX_WIDTHS))
        B, M, W = (int(v) for v in gt_boxes.shape)
        if not 0 < B <= _lib.AUG_MAX_BATCH:
            raise ValueError('batch of %d frames: the augmentation kernels take 1 to %d' % (B, _lib.AUG_MAX_BATCH))
        n_sweeps = tf_rows = 0
        if instances_tf is not None:
            if instances_tf.dim() != 5 or tuple(instances_tf.shape[:2]) != (B, M) or instances_tf.shape[3] not in TF_ROWS or instances_tf.shape[4] != 4:
                raise ValueError('instances_tf of shape %s: the augmentation kernel takes (B, M, S, R, 4) with R in %s and (B, M) = (%d, %d) '
                                 'of gt_boxes' % (tuple(instances_tf.shape), TF_ROWS, B, M))
            n_sweeps, tf_rows = int(instances_tf.shape[2]), int(instances_tf.shape[3])
            instances_tf = instances_tf.float().contiguous().clone()
        gt_boxes = gt_boxes.float().contiguous().clone()
        a = self.descriptor(B, stages, False)
        if M > 0 and (instances_tf is None or n_sweeps > 0):
            check(_lib.load().pcp_world_augment_boxes(ctypes.byref(a), _p(table_dev), _p(gt_boxes), M, W, _p(instances_tf), n_sweeps, tf_rows,
                                                      _stream()), 'pcp_world_augment_boxes')
        return gt_boxes, instances_tf

    def apply(self, batch_dict, params):
        """augments batch_dict in place (new tensors under the same keys): points, gt_boxes, instances_tf, metadata[*]['se3_from_ego'], and
        stores flip_x / flip_y / noise_rot / noise_scale per frame as the reference's collated batch carries them"""
        B = int(batch_dict['batch_size'])
        assert len(params['flip_x']) == B, (len(params['flip_x']), B)
        if self.gt_sampler is not None:                      # the paste first: pasted points and boxes go through the transforms and the mask
            self.gt_sampler.apply(batch_dict, params['gt_sampled'])
        points = batch_dict['points']
        _need_cuda(points)
        table_dev = torch.from_numpy(self.table(params)).to(points.device)
        batch_dict['points'], kept = self.augment_points(points, table_dev, B)
        if kept is not None:
            batch_dict['aug_points_kept'] = kept
        if batch_dict.get('gt_boxes', None) is not None:
            batch_dict['gt_boxes'], tf = self.augment_boxes(batch_dict['gt_boxes'], batch_dict.get('instances_tf', None), table_dev)
            if tf is not None:
                batch_dict['instances_tf'] = tf
        elif batch_dict.get('instances_tf', None) is not None:
            raise ValueError('instances_tf without gt_boxes: the class column of gt_boxes tells the real objects from the padding')
        meta = batch_dict.get('metadata', None)
        if meta is not None:
            batch_dict['metadata'] = [dict(m, se3_from_ego=augment_se3_from_ego(m['se3_from_ego'], self.stages, params, b))
                                      if isinstance(m, dict) and 'se3_from_ego' in m else m for b, m in enumerate(meta)]
        names = {n for n, _ in self.queue}
        if 'random_world_flip' in names:
            for st, key in ((_lib.AUG_FLIP_X, 'flip_x'), (_lib.AUG_FLIP_Y, 'flip_y')):
                if st in self.stages:
                    batch_dict[key] = np.asarray(params[key]).copy()
        if 'random_world_rotation' in names:
            batch_dict['noise_rot'] = np.asarray(params['noise_rot']).copy()
        if 'random_world_scaling' in names:
            batch_dict['noise_scale'] = np.asarray(params['noise_scale']).copy()
        return batch_dict

    def __call__(self, batch_dict, rng=None):
        classes = self.gt_sampler.frame_gt_classes(batch_dict['gt_boxes']) if self.gt_sampler is not None else None
        return self.apply(batch_dict, self.draw(batch_dict['batch_size'], self.rng if rng is None else rng, classes))
