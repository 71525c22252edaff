"""What the augmentation drivers share (augment.py, object_augment.py, gt_sampler.py): the config getter, the refusals of point rows and
of instances_tf, and the one points launch of csrc/augment.hip and csrc/object_augment.hip that may filter rows (csrc/aug_tile.h)."""
import torch

from . import lib as _lib
from .lib import check
from .ops import _p, _stream

BOX_WIDTHS = (8, 10)                 # [x y z dx dy dz heading class] / [.. heading vx vy class]
TF_ROWS = (3, 4)                     # instances_tf (B, M, S, 3 | 4, 4)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def check_rows(points, batch_size, what):
    """the refusals of the rows of a points launch, `what` names the caller in them -> the rows contiguous and 16-byte aligned"""
    if points.dim() != 2 or not _lib.AUG_MIN_ROW_STRIDE <= points.shape[1] <= _lib.AUG_MAX_ROW_STRIDE:
        raise ValueError('points of shape %s: %s takes (N, 1 + C) rows of %d (frame index, x y z) up to %d columns'
                         % (tuple(points.shape), what, _lib.AUG_MIN_ROW_STRIDE, _lib.AUG_MAX_ROW_STRIDE))
    if points.dtype != torch.float32:
        raise ValueError('points are %s: %s reads float32 rows' % (points.dtype, what))
    if not 0 < batch_size <= _lib.AUG_MAX_BATCH:
        raise ValueError('batch of %d frames: the augmentation kernels take 1 to %d' % (batch_size, _lib.AUG_MAX_BATCH))
    if not points.is_cuda:
        return points                                   # the caller's _need_cuda refuses it once every argument has been looked at
    points = points.contiguous()
    return points.clone() if points.data_ptr() % 16 else points


def check_instances_tf(instances_tf, B, M):
    """-> (sweeps, rows) of instances_tf (B, M, S, 3 | 4, 4)"""
    if instances_tf.dim() != 5 or tuple(instances_tf.shape[:2]) != (B, M) or instances_tf.shape[3] not in TF_ROWS or instances_tf.shape[4] != 4:
        raise ValueError('instances_tf of shape %s: the augmentation kernel takes (B, M, S, R, 4) with R in %s and (B, M) = (%d, %d) '
                         'of gt_boxes' % (tuple(instances_tf.shape), TF_ROWS, B, M))
    return int(instances_tf.shape[2]), int(instances_tf.shape[3])


def points_call(launch, workspace_bytes, head, points, slots):
    """launch: pcp_world_augment_points | pcp_object_augment_points of the loaded library, workspace_bytes: its *_workspace_bytes, head: its
    arguments in front of `points`; on checked rows.  slots = 0: no row is dropped -> (a new tensor of all rows, None), nothing read back.
    Otherwise the call filters: workspace, `slots` int32 counters, one host read of them -> (a new tensor holding the kept rows in input
    order, the counters as a numpy array)."""
    n, stride = int(points.shape[0]), int(points.shape[1])
    out = torch.empty_like(points)
    counts = ws = None
    ws_bytes = 0
    if slots:
        ws_bytes = int(workspace_bytes(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=points.device)
        counts = torch.empty(slots, dtype=torch.int32, device=points.device)
    check(launch(*head, _p(points), n, stride, _p(out), _p(counts), _p(ws), ws_bytes, _stream()), launch.__name__)
    if not slots:
        return out, None
    kept = counts.cpu().numpy()
    return out[:int(kept.sum())], kept
