"""World augmentation of a collated training batch on the device (csrc/augment.hip).

The reference augments every sample in its DataLoader workers (pcdet/datasets/augmentor/data_augmentor.py, augmentor_utils.py: numpy and
torch-CPU) and masks the points outside the range afterwards (data_processor.py mask_points_and_boxes_outside_range).  Here the batch
is collated and on the GPU already, so DeviceWorldAugmentor

  * parses DATA_AUGMENTOR the way DataAugmentor.__init__ does and keeps the four world transforms in list order (random_world_flip,
    random_world_rotation, random_world_scaling, random_world_translation); gt_sampling runs in front of them when a DeviceGtSampler is given
    (pcp_amd/gt_sampler.py: it holds the database); every other entry (the local augmentations and dropouts need RoI data, ...) is
    skipped with one logged line; object_stages=True also takes the per-object entries (random_local_translation / _rotation / _scaling,
    random_local_frustum_dropout, random_world_frustum_dropout: pcp_amd/object_augment.py) in list order;
  * draw(): draws, frame by frame, exactly the numpy calls the reference makes for consecutive samples;
  * apply(): the launches of self.steps on the current stream (a list of world transforms is one step of two launches: points; gt_boxes +
    instances_tf) and the float64 se3_from_ego update on the host.

There is no CPU path: apply() needs CUDA tensors.
"""
import ctypes
import logging
import math

import numpy as np
import torch

from . import lib as _lib
from . import object_augment as _obj
from .aug_common import BOX_WIDTHS, _get, check_instances_tf, check_rows, points_call
from .lib import check
from .ops import _need_cuda, _p, _stream

WORLD_TRANSFORMS = ('random_world_flip', 'random_world_rotation', 'random_world_scaling', 'random_world_translation')
RANGE_FILTER = 'mask_points_and_boxes_outside_range'
GT_SAMPLING = 'gt_sampling'


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
    the boxes); gt_sampler: a DeviceGtSampler, without one a gt_sampling entry is skipped like the other entries the device path lacks;
    object_stages: the per-object entries (object_augment.OBJECT_STAGES) join the queue instead of being skipped."""

    def __init__(self, aug_cfg, point_cloud_range, layout='car', data_processor=None, logger=None, seed=None, gt_sampler=None,
                 object_stages=False):
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
            if object_stages and name in _obj.OBJECT_STAGES:
                self.queue.append((name, cur))
                continue
            if name not in WORLD_TRANSFORMS:
                self.skipped.append(name)
                self.logger.info('DeviceWorldAugmentor: %s is not a world transform of the device path, skipped' % name)
                continue
            self.queue.append((name, cur))
        self.stages = []                   # PCP_AUG_* in the order the kernels apply them
        for name, cur in self.queue:
            if name == GT_SAMPLING or name in _obj.OBJECT_STAGES:
                continue
            self.stages.extend(self.world_stage_codes(name, cur))
        if len(self.stages) > _lib.AUG_MAX_STAGES:
            raise ValueError('%d augmentation stages: the kernels take %d' % (len(self.stages), _lib.AUG_MAX_STAGES))
        self.has_object_stages = any(name in _obj.OBJECT_STAGES for name, _ in self.queue)
        self._plan()

    @staticmethod
    def world_stage_codes(name, cur):
        if name == 'random_world_flip':
            out = []
            for axis in _get(cur, 'ALONG_AXIS_LIST'):
                assert axis in ('x', 'y'), axis
                out.append(_lib.AUG_FLIP_X if axis == 'x' else _lib.AUG_FLIP_Y)
            return out
        return [{'random_world_rotation': _lib.AUG_ROTATE, 'random_world_scaling': _lib.AUG_SCALE,
                 'random_world_translation': _lib.AUG_TRANSLATE}[name]]

    def _plan(self):
        """the launches in list order.  self.steps: dicts(kind 'gt' | 'world' | 'local' | 'wdrop', q: queue indices, stages).  Consecutive
        world entries share one call of the world kernels, consecutive local entries one of the object kernels.  self.splits: queue
        indices in front of which the per-frame box counts must be read back before the draws go on, i.e. the first object entry behind
        an enabled gt_sampling or a world frustum dropout."""
        self.steps, self.splits = [], []
        if not self.has_object_stages:                  # the paste, then every world entry in one call of the world kernels
            world = [qi for qi, (name, _) in enumerate(self.queue) if name != GT_SAMPLING]
            self.steps = [{'kind': 'gt', 'q': [qi], 'stages': []} for qi in range(len(self.queue)) if qi not in world]
            self.steps.append({'kind': 'world', 'q': world, 'stages': list(self.stages)})
            return
        changed = False                                 # a device stage has changed the box counts since the last read
        for qi, (name, cur) in enumerate(self.queue):
            if name == GT_SAMPLING:
                if any(n in _obj.OBJECT_STAGES for n, _ in self.queue[:qi]):
                    # apply() pastes in front of every other stage, and the draws of an earlier object stage cover the original boxes only
                    raise ValueError('gt_sampling behind %s: the device path pastes first, so gt_sampling must stand in front of every '
                                     'per-object stage of the list' % [n for n, _ in self.queue[:qi] if n in _obj.OBJECT_STAGES][0])
                self.steps.append({'kind': 'gt', 'q': [qi], 'stages': []})
                changed = True
                continue
            if name in _obj.LOCAL_STAGES:
                if changed:
                    self.splits.append(qi)
                    changed = False
                subs = [c for c, _, _ in _obj.sub_stages(name, cur)]
                last = self.steps[-1] if self.steps else None
                if last is not None and last['kind'] == 'local' and qi not in self.splits and len(last['stages']) + len(subs) <= _lib.OBJ_MAX_STAGES:
                    last['q'].append(qi)
                    last['stages'].extend(subs)
                else:
                    self.steps.append({'kind': 'local', 'q': [qi], 'stages': subs})
            elif name == _obj.WORLD_DROPOUT:
                self.steps.append({'kind': 'wdrop', 'q': [qi], 'stages': [c for c, _, _ in _obj.sub_stages(name, cur)]})
                changed = True
            else:
                codes = self.world_stage_codes(name, cur)
                last = self.steps[-1] if self.steps else None
                if last is not None and last['kind'] == 'world':
                    last['q'].append(qi)
                    last['stages'].extend(codes)
                else:
                    self.steps.append({'kind': 'world', 'q': [qi], 'stages': codes})
        # the heading's limit_period and the range mask come once, behind the whole list
        if self.steps[-1]['kind'] != 'world' and (self.filter or self.steps[-1]['kind'] != 'local'):
            self.steps.append({'kind': 'world', 'q': [], 'stages': []})

    @classmethod
    def from_dataset_cfg(cls, dataset_cfg, layout='car', logger=None, seed=None, gt_sampler=None, object_stages=False):
        return cls(dataset_cfg.DATA_AUGMENTOR, dataset_cfg.POINT_CLOUD_RANGE, layout, data_processor=_get(dataset_cfg, 'DATA_PROCESSOR', []),
                   logger=logger, seed=seed, gt_sampler=gt_sampler, object_stages=object_stages)

    @staticmethod
    def rot_range(cur):
        r = _get(cur, 'WORLD_ROT_ANGLE')
        return [-r, r] if not isinstance(r, (list, tuple)) else list(r)

    def draw(self, batch_size, rng, gt_classes=None, n_boxes=None, entries=None, params=None):
        """rng: numpy.random.RandomState.  Frame after frame, the calls the reference makes on numpy's global generator for consecutive
        samples, in its order; with RandomState(s) the parameters equal the reference's after np.random.seed(s).  With a gt sampler,
        gt_classes[b] are the class ids of frame b's original boxes and the sampler's draws for frame b come before its world draws.
        With object stages n_boxes[b] is the number of real boxes of frame b (one uniform per box and sub-stage); their values land in
        p['object'][queue index][b].  entries = (lo, hi) draws only the queue entries lo .. hi - 1 into `params` (__call__ uses it when the
        box counts have to be read back in the middle of the list)."""
        B = int(batch_size)
        if self.has_object_stages and (n_boxes is None or len(n_boxes) != B):
            raise ValueError('draw() with object stages needs n_boxes, the number of real boxes of each of the %d frames' % B)
        lo_q, hi_q = entries if entries is not None else (0, len(self.queue))
        if params is not None:
            p = params
            for b in range(B):
                self._draw_frame(b, rng, p, gt_classes, n_boxes, lo_q, hi_q)
            return p
        if self.gt_sampler is not None and (gt_classes is None or len(gt_classes) != B):
            raise ValueError('draw() with a gt sampler needs gt_classes, the class ids of the original boxes of each of the %d frames' % B)
        p = {'flip_x': np.zeros(B, dtype=bool), 'flip_y': np.zeros(B, dtype=bool), 'noise_rot': np.zeros(B, dtype=np.float64),
             'noise_scale': np.ones(B, dtype=np.float64), 'noise_translate': np.zeros((B, 3), dtype=np.float32)}
        if self.gt_sampler is not None:
            p['gt_sampled'] = []
        if self.has_object_stages:
            p['object'] = {qi: [None] * B for qi, (name, _) in enumerate(self.queue) if name in _obj.OBJECT_STAGES}
        for b in range(B):
            self._draw_frame(b, rng, p, gt_classes, n_boxes, lo_q, hi_q)
        return p

    def _draw_frame(self, b, rng, p, gt_classes, n_boxes, lo_q, hi_q):
        if self.gt_sampler is not None and lo_q == 0:
            p['gt_sampled'].append(self.gt_sampler.draw(gt_classes[b], rng))
        for qi, (name, cur) in enumerate(self.queue):
            if name == GT_SAMPLING or not lo_q <= qi < hi_q:
                continue
            if name in _obj.OBJECT_STAGES:
                p['object'][qi][b] = _obj.draw_entry(name, cur, n_boxes[b], rng)
            elif name == 'random_world_flip':
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

    def descriptor(self, batch_size, stages=None, filter=None, raw_heading=False):
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
        a.raw_heading = int(bool(raw_heading))
        return a

    # ---- the two launches ---------------------------------------------------------------------------------------------------------
    def augment_points(self, points, table_dev, batch_size, stages=None, filter=None):
        """points (N, 1 + C) float32 CUDA -> (rows, per-frame kept counts as a numpy array or None).  Filter on: a new tensor holding the
        kept rows in input order (one host read of 4 B bytes); filter off: a new tensor of all N rows, nothing read back."""
        _need_cuda(points, table_dev)
        points = check_rows(points, batch_size, 'the augmentation kernel')
        if self.hd_map and points.shape[1] != 13:
            raise ValueError('HD-map rows have 1 + 12 columns, got %d' % points.shape[1])
        a = self.descriptor(batch_size, stages, filter)
        L = _lib.load()
        return points_call(L.pcp_world_augment_points, L.pcp_world_augment_points_workspace_bytes, (ctypes.byref(a), _p(table_dev)), points,
                           batch_size if a.filter else 0)

    def augment_boxes(self, gt_boxes, instances_tf, table_dev, stages=None, raw_heading=False):
        """gt_boxes (B, M, 8 | 10), instances_tf (B, M, S, 3 | 4, 4) or None -> new tensors; one launch.  raw_heading: no limit_period at the
        end (object stages follow)"""
        _need_cuda(gt_boxes, instances_tf, table_dev)
        if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in BOX_WIDTHS:
            raise ValueError('gt_boxes of shape %s: the augmentation kernel takes (B, M, W) with W in %s (x y z dx dy dz heading [vx vy] class)'
                             % (tuple(gt_boxes.shape), BOX_WIDTHS))
        B, M, W = (int(v) for v in gt_boxes.shape)
        if not 0 < B <= _lib.AUG_MAX_BATCH:
            raise ValueError('batch of %d frames: the augmentation kernels take 1 to %d' % (B, _lib.AUG_MAX_BATCH))
        n_sweeps = tf_rows = 0
        if instances_tf is not None:
            n_sweeps, tf_rows = check_instances_tf(instances_tf, B, M)
            instances_tf = instances_tf.float().contiguous().clone()
        gt_boxes = gt_boxes.float().contiguous().clone()
        a = self.descriptor(B, stages, False, raw_heading)
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
        self.run_steps(batch_dict, params, [s for s in self.steps if s['kind'] != 'gt'])
        return self._finish(batch_dict, params)

    def run_steps(self, batch_dict, params, steps):
        """the launches of `steps` (self.steps entries other than the paste) on batch_dict, in order"""
        B = int(batch_dict['batch_size'])
        self.check_plan(batch_dict, steps)
        _need_cuda(batch_dict['points'])
        table_dev = torch.from_numpy(self.table(params)).to(batch_dict['points'].device)
        for step in steps:
            final = step is self.steps[-1]
            if step['kind'] == 'world':
                filt = self.filter and final
                # a list without object stages always launches: the caller gets a new tensor, never its own
                if step['stages'] or filt or not self.has_object_stages:
                    batch_dict['points'], kept = self.augment_points(batch_dict['points'], table_dev, B, stages=step['stages'], filter=filt)
                    if kept is not None:
                        batch_dict['aug_points_kept'] = kept
                if batch_dict.get('gt_boxes', None) is not None:
                    batch_dict['gt_boxes'], tf = self.augment_boxes(batch_dict['gt_boxes'], batch_dict.get('instances_tf', None), table_dev,
                                                                    stages=step['stages'], raw_heading=not final)
                    if tf is not None:
                        batch_dict['instances_tf'] = tf
                elif batch_dict.get('instances_tf', None) is not None:
                    raise ValueError('instances_tf without gt_boxes: the class column of gt_boxes tells the real objects from the padding')
            elif step['kind'] == 'local':
                if not step['stages']:
                    continue
                values = [np.concatenate([np.asarray(params['object'][qi][b], dtype=np.float64).reshape(len(_obj.sub_stages(*self.queue[qi])), -1)
                                          for qi in step['q'] if len(_obj.sub_stages(*self.queue[qi]))], axis=0) for b in range(B)]
                batch_dict['points'], batch_dict['gt_boxes'], _ = _obj.local_stages(batch_dict['points'], batch_dict['gt_boxes'].float(),
                                                                                    step['stages'], values, limit_heading=final)
            elif step['kind'] == 'wdrop':
                qi = step['q'][0]
                for k, direction in enumerate(step['stages']):
                    inten = [float(np.asarray(params['object'][qi][b]).reshape(-1)[k]) for b in range(B)]
                    batch_dict['points'], batch_dict['gt_boxes'], tf, _, _ = _obj.world_dropout(
                        batch_dict['points'], batch_dict['gt_boxes'].float(), batch_dict.get('instances_tf', None), direction, inten)
                    if tf is not None:
                        batch_dict['instances_tf'] = tf

    @staticmethod
    def check_plan(batch_dict, steps):
        """the refusals of every object step of `steps`, before the first launch of any of them: no world stage changes the dtype, the box
        width or the number of box rows, so what holds for the batch as it arrives holds at each step"""
        stages = [c for s in steps if s['kind'] in ('local', 'wdrop') for c in s['stages']]
        if not stages:
            return
        if batch_dict.get('gt_boxes', None) is None:
            raise ValueError('object stages need gt_boxes: they move the points inside each box')
        gt, pts = batch_dict['gt_boxes'], batch_dict['points']
        _obj._check_boxes(gt.float(), stages)                    # run_steps hands the boxes over as float32
        check_rows(pts, int(batch_dict['batch_size']), _obj.WHAT)

    def _finish(self, batch_dict, params):
        if self.gt_sampler is not None or self.has_object_stages:
            batch_dict.pop('num_gt_boxes', None)            # the loader's counts: the paste and the world dropout have changed them
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

    @staticmethod
    def box_counts(batch_dict):
        """the real boxes of every frame: batch_dict['num_gt_boxes'] when the loader put the host's numbers there, else one read of the class
        column's per-frame counts (B integers)"""
        if batch_dict.get('num_gt_boxes', None) is not None:
            return [int(v) for v in batch_dict['num_gt_boxes']]
        return [int(v) for v in (batch_dict['gt_boxes'][..., -1] != 0).sum(dim=1).cpu().tolist()]

    def __call__(self, batch_dict, rng=None):
        rng = self.rng if rng is None else rng
        classes = self.gt_sampler.frame_gt_classes(batch_dict['gt_boxes']) if self.gt_sampler is not None else None
        B = int(batch_dict['batch_size'])
        n_boxes = None
        if self.has_object_stages:
            n_boxes = [len(c) for c in classes] if classes is not None else self.box_counts(batch_dict)
        # where the box counts change on the device in the middle of the list: draw up to there, run, read the counts back (once per such place), go on
        bounds = [0] + self.splits + [len(self.queue)]
        params = None
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if lo > 0:
                batch_dict.pop('num_gt_boxes', None)
                n_boxes = self.box_counts(batch_dict)
            params = self.draw(B, rng, classes, n_boxes, (lo, hi), params)
            if lo == 0 and self.gt_sampler is not None:
                self.gt_sampler.apply(batch_dict, params['gt_sampled'])
            steps = [s for s in self.steps if s['kind'] != 'gt' and (all(lo <= q < hi for q in s['q']) if s['q'] else hi == len(self.queue))]
            self.run_steps(batch_dict, params, steps)
        return self._finish(batch_dict, params)
