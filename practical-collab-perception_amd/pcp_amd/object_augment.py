"""Per-object augmentation of a collated training batch on the device (csrc/object_augment.hip): the reference's random_local_translation,
random_local_rotation, random_local_scaling, random_local_frustum_dropout and random_world_frustum_dropout (data_augmentor.py,
augmentor_utils.py).  DeviceWorldAugmentor(object_stages=True) puts them in its queue; this module holds what is theirs alone: how a
config entry becomes sub-stages, the reference's draws, and the launches.

A local entry becomes one sub-stage per axis / direction; consecutive local entries share one launch pair (boxes, points).  A world
frustum dropout direction is three calls: pcp_frame_extent, pcp_object_augment_drop_boxes (threshold and box filter), and the row filter.
Every call with a dropout reads its per-frame kept counts back (B integers), as the range mask of the world path does.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .aug_common import _get, check_instances_tf, check_rows, points_call
from .lib import check
from .ops import _need_cuda, _p, _stream

LOCAL_STAGES = ('random_local_translation', 'random_local_rotation', 'random_local_scaling', 'random_local_frustum_dropout')
WORLD_DROPOUT = 'random_world_frustum_dropout'
OBJECT_STAGES = LOCAL_STAGES + (WORLD_DROPOUT,)
DIRECTIONS = ('top', 'bottom', 'left', 'right')
_TRANSLATE = {'x': _lib.OBJ_TRANSLATE_X, 'y': _lib.OBJ_TRANSLATE_Y, 'z': _lib.OBJ_TRANSLATE_Z}
_LOCAL_DROP = dict(zip(DIRECTIONS, (_lib.OBJ_DROP_TOP, _lib.OBJ_DROP_BOTTOM, _lib.OBJ_DROP_LEFT, _lib.OBJ_DROP_RIGHT)))
_WORLD_DROP = dict(zip(DIRECTIONS, (_lib.OBJ_WORLD_DROP_TOP, _lib.OBJ_WORLD_DROP_BOTTOM, _lib.OBJ_WORLD_DROP_LEFT, _lib.OBJ_WORLD_DROP_RIGHT)))
_DROPS = set(_LOCAL_DROP.values()) | set(_WORLD_DROP.values())
WHAT = 'the object augmentation'                        # how check_rows names this module in its refusals


def sub_stages(name, cur):
    """-> [(PCP_OBJ_* code, lo, hi)] of one config entry: the uniform range of every sub-stage, in the reference's order.  An empty list:
    the entry does nothing and draws nothing (local_scaling returns early when hi - lo < 1e-3)."""
    if name == 'random_local_translation':
        lo, hi = _get(cur, 'LOCAL_TRANSLATION_RANGE')
        out = []
        for axis in _get(cur, 'ALONG_AXIS_LIST'):
            assert axis in ('x', 'y', 'z'), axis
            out.append((_TRANSLATE[axis], lo, hi))
        return out
    if name == 'random_local_rotation':
        r = _get(cur, 'LOCAL_ROT_ANGLE')
        lo, hi = list(r) if isinstance(r, (list, tuple)) else (-r, r)
        return [(_lib.OBJ_ROTATE, lo, hi)]
    if name == 'random_local_scaling':
        lo, hi = _get(cur, 'LOCAL_SCALE_RANGE')
        return [] if hi - lo < 1e-3 else [(_lib.OBJ_SCALE, lo, hi)]
    table = _LOCAL_DROP if name == 'random_local_frustum_dropout' else _WORLD_DROP
    lo, hi = _get(cur, 'INTENSITY_RANGE')
    out = []
    for d in _get(cur, 'DIRECTION'):
        assert d in DIRECTIONS, d
        out.append((table[d], lo, hi))
    return out


def draw_entry(name, cur, n_boxes, rng):
    """the reference's numpy calls of one entry on one sample: per sub-stage one rng.uniform(lo, hi) per box (local) or one in all (world
    dropout) -> float64 (n_sub, n_boxes) / (n_sub,)"""
    subs = sub_stages(name, cur)
    if name == WORLD_DROPOUT:
        return np.asarray([rng.uniform(lo, hi) for _, lo, hi in subs], dtype=np.float64)
    return np.asarray([[rng.uniform(lo, hi) for _ in range(int(n_boxes))] for _, lo, hi in subs], dtype=np.float64).reshape(len(subs), int(n_boxes))


def descriptor(stages, batch_size, limit_heading=False):
    if len(stages) > _lib.OBJ_MAX_STAGES:
        raise ValueError('%d object sub-stages in one call: the kernels take %d' % (len(stages), _lib.OBJ_MAX_STAGES))
    a = _lib.ObjectAug()
    a.n_stages = len(stages)
    for i, s in enumerate(stages):
        a.stage[i] = int(s)
    a.batch = int(batch_size)
    a.limit_heading = int(bool(limit_heading))
    return a


def param_table(stages, values, max_boxes):
    """stages: PCP_OBJ_* codes; values: per frame a float64 (n_sub, n_b) array -> (B, n_sub, max_boxes, OBJ_PARAM_STRIDE) float32.  cos / sin
    of a rotation are torch's float32 values of the float32 angle (augment.rotation_cos_sin), as the world rotation takes them."""
    from .augment import rotation_cos_sin
    B, K = len(values), len(stages)
    t = np.zeros((B, K, max_boxes, _lib.OBJ_PARAM_STRIDE), dtype=np.float32)
    for b, v in enumerate(values):
        v = np.asarray(v, dtype=np.float64).reshape(K, -1)
        nb = v.shape[1]
        if nb > max_boxes:
            raise ValueError('frame %d: parameters for %d boxes, gt_boxes holds %d rows' % (b, nb, max_boxes))
        t[b, :, :nb, 0] = v.astype(np.float32)
        for k, st in enumerate(stages):
            if st == _lib.OBJ_ROTATE:
                t[b, k, :nb, 1], t[b, k, :nb, 2] = rotation_cos_sin(v[k])
    return t


def _check_boxes(gt_boxes, stages=()):
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in (8, 10):
        raise ValueError('gt_boxes of shape %s: the object augmentation takes (B, M, 8 | 10)' % (tuple(gt_boxes.shape),))
    if gt_boxes.dtype != torch.float32:
        raise ValueError('gt_boxes are %s: the object augmentation reads float32 rows' % gt_boxes.dtype)
    if gt_boxes.shape[1] > _lib.OBJ_MAX_BOXES:
        raise ValueError('gt_boxes hold %d rows per frame: the object augmentation takes at most %d (PCP_OBJ_MAX_BOXES)'
                         % (gt_boxes.shape[1], _lib.OBJ_MAX_BOXES))
    if gt_boxes.shape[2] == 10 and _lib.OBJ_ROTATE in stages:
        raise ValueError('random_local_rotation with 10-column boxes: the reference\'s own velocity branch (augmentor_utils.local_rotation) '
                         'raises on them, so there is nothing to reproduce')


def _points_call(a, states, n_boxes, max_boxes, frame_thr, points):
    """-> (rows, per-frame kept counts as numpy or None)"""
    drop = any(a.stage[i] in _DROPS for i in range(a.n_stages))
    head = (ctypes.byref(a), _p(states), _p(n_boxes), int(max_boxes), _p(frame_thr))
    L = _lib.load()
    # counter [batch]: rows of a frame outside [0, batch), kept
    out, kept = points_call(L.pcp_object_augment_points, L.pcp_object_augment_points_workspace_bytes, head, points, a.batch + 1 if drop else 0)
    return out, None if kept is None else kept[:a.batch]


def local_stages(points, gt_boxes, stages, values, limit_heading=False):
    """The local sub-stages `stages` on points (N, 1 + C) and gt_boxes (B, M, 8 | 10), float32 CUDA; values: per frame the drawn
    (n_sub, n_b) array.  -> (points, gt_boxes, per-frame kept counts or None): new tensors, the inputs are not written."""
    _check_boxes(gt_boxes, stages)
    B, M, W = (int(v) for v in gt_boxes.shape)
    points = check_rows(points, B, WHAT)
    _need_cuda(points, gt_boxes)
    if len(values) != B:
        raise ValueError('parameters for %d frames, gt_boxes has %d' % (len(values), B))
    a = descriptor(stages, B, limit_heading)
    dev = points.device
    gt_boxes = gt_boxes.contiguous().clone()
    params = torch.from_numpy(param_table(stages, values, M)).to(dev)
    states = torch.empty((B, max(len(stages), 1), max(M, 1), _lib.OBJ_STATE_STRIDE), dtype=torch.float32, device=dev)
    n_boxes = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.load().pcp_object_augment_boxes(ctypes.byref(a), _p(params), _p(gt_boxes), M, W, _p(states), _p(n_boxes), _stream()),
          'pcp_object_augment_boxes')
    out, kept = _points_call(a, states, n_boxes, M, None, points)
    return out, gt_boxes, kept


def frame_extent(points, batch_size, col):
    """(B, 2) float32 CUDA: min, max of column `col` per frame; +inf, -inf for a frame without rows"""
    points = check_rows(points, batch_size, WHAT)
    _need_cuda(points)
    L = _lib.load()
    n = int(points.shape[0])
    ws_bytes = int(L.pcp_frame_extent_workspace_bytes(n, batch_size))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=points.device)
    extent = torch.empty((batch_size, 2), dtype=torch.float32, device=points.device)
    check(L.pcp_frame_extent(_p(points), n, int(points.shape[1]), batch_size, int(col), _p(extent), _p(ws), ws_bytes, _stream()), 'pcp_frame_extent')
    return extent


def world_dropout(points, gt_boxes, instances_tf, direction, intensity):
    """One direction (PCP_OBJ_WORLD_DROP_*) of random_world_frustum_dropout with the drawn per-frame intensity (B,).
    -> (points, gt_boxes, instances_tf, per-frame kept rows, per-frame box counts as a CUDA int32 tensor)"""
    _check_boxes(gt_boxes)
    B, M, W = (int(v) for v in gt_boxes.shape)
    points = check_rows(points, B, WHAT)
    _need_cuda(points, gt_boxes)
    dev = points.device
    col = 3 if direction in (_lib.OBJ_WORLD_DROP_TOP, _lib.OBJ_WORLD_DROP_BOTTOM) else 2
    extent = frame_extent(points, B, col)
    inten = torch.from_numpy(np.asarray(intensity, dtype=np.float64).astype(np.float32).reshape(B)).to(dev)
    thr = torch.empty(B, dtype=torch.float32, device=dev)
    n_out = torch.empty(B, dtype=torch.int32, device=dev)
    gt_boxes = gt_boxes.contiguous()
    gt_out = torch.empty_like(gt_boxes)
    n_sweeps = tf_rows = 0
    tf_out = None
    if instances_tf is not None:
        _need_cuda(instances_tf)
        n_sweeps, tf_rows = check_instances_tf(instances_tf, B, M)
        instances_tf = instances_tf.float().contiguous()
        tf_out = torch.empty_like(instances_tf) if n_sweeps > 0 else instances_tf
    check(_lib.load().pcp_object_augment_drop_boxes(_p(gt_boxes), B, M, W, _p(instances_tf) if n_sweeps else None, n_sweeps, tf_rows, _p(extent),
                                                    _p(inten), int(direction), _p(thr), _p(gt_out), _p(tf_out) if n_sweeps else None,
                                                    _p(n_out), _stream()), 'pcp_object_augment_drop_boxes')
    out, kept = _points_call(descriptor([direction], B), None, None, 0, thr, points)
    return out, gt_out, tf_out, kept, n_out
