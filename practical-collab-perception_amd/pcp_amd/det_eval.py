"""Detection evaluation by the nuScenes protocol on the device (csrc/det_eval.hip).

The reference hands its detections to nuscenes-devkit on the host (pcdet/datasets/v2x_sim/v2x_sim_eval_utils.py,
pcdet/datasets/nuscenes/nuscenes_eval_utils.py): greedy matching of predictions to ground truth by centre distance, per class, at
0.5 / 1 / 2 / 4 m; AP from a 101-point precision curve; translation / scale / orientation / velocity errors over the matches at 2 m.  Here

  * DeviceDetectionEval.add() pads the detector's final per-frame dicts into (B, K, .) tensors with torch ops and launches
    pcp_det_eval_match: one 32-byte record per prediction slot of an epoch buffer, one ground-truth count per (frame, class).  Nothing is
    read back (when a frame can hold more than EVAL_MAX_BOXES boxes, the per-class counts are checked first, which is one small read);
  * result() orders the epoch's records per class by score (two stable torch sorts), launches pcp_det_eval_curves and reads its output --
    per class 3 x 4 x 101 doubles and a few counts -- which is the one read of an evaluation.  AP, the TP means, mAP and NDS are finished
    from those arrays in float64 numpy.

Attribute error, the devkit's class-range and point-count filters and KITTI-style AP are not computed.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .lib import check
from .ops import _p, _stream

METRICS = ('trans_err', 'scale_err', 'orient_err', 'vel_err')


def class_protocol(name):
    """-> (orientation period, flags) of a class name: barriers are symmetric under a half turn and have no velocity, cones have neither"""
    period = np.pi if name == 'barrier' else 2.0 * np.pi
    flags = 0
    if name == 'traffic_cone':
        flags = _lib.EVAL_NAN_ORIENT | _lib.EVAL_NAN_VEL
    elif name == 'barrier':
        flags = _lib.EVAL_NAN_VEL
    return period, flags


def format_results(metrics, class_names, version='default'):
    """the text block the reference logs after an evaluation (layout of its format_nuscene_results): one header and one value line per
    class, then the averages"""
    lines = ['----------------Nuscene %s results-----------------' % version]
    for name in class_names:
        aps, errs = metrics['label_aps'][name], metrics['label_tp_errors'][name]
        lines.append('***%s error@%s | AP@%s' % (name, ', '.join(k.split('_')[0] for k in errs), ', '.join('%s' % d for d in aps)))
        lines.append('%s | %s | mean AP: %s' % (', '.join('%.2f' % v for v in errs.values()), ', '.join('%.2f' % (100.0 * v) for v in aps.values()),
                                                metrics['mean_dist_aps'][name]))
    lines.append('--------------average performance-------------')
    for key, val in metrics['tp_errors'].items():
        lines.append('%s:\t %.4f' % (key, val))
    lines.append('mAP:\t %.4f' % metrics['mean_ap'])
    if 'nd_score' in metrics:
        lines.append('NDS:\t %.4f' % metrics['nd_score'])
    return '\n'.join(lines) + '\n'


class DeviceDetectionEval:
    """class_names: the model's classes (label l of a prediction and class l of a gt row mean class_names[l - 1]); max_boxes: detections
    kept per frame (the top ones by score, the devkit's cap) = slots per frame of the epoch buffer; capacity_frames: frames per epoch."""

    def __init__(self, class_names, dist_ths=(0.5, 1, 2, 4), dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, max_boxes=500, capacity_frames=1024):
        self.class_names = [str(n) for n in class_names]
        self.dist_ths = tuple(float(d) for d in dist_ths)
        if len(self.dist_ths) != _lib.EVAL_THRESHOLDS:
            raise ValueError('%d distance thresholds: the match kernel runs one wave for each of exactly %d' % (len(self.dist_ths), _lib.EVAL_THRESHOLDS))
        if float(dist_th_tp) not in self.dist_ths:
            raise ValueError('dist_th_tp %g is not one of dist_ths %s' % (dist_th_tp, self.dist_ths))
        if not self.class_names or int(max_boxes) <= 0 or int(capacity_frames) <= 0:
            raise ValueError('class_names, max_boxes and capacity_frames must not be empty / zero')
        self.tp_index = self.dist_ths.index(float(dist_th_tp))
        self.dist_th_tp = float(dist_th_tp)
        self.min_recall, self.min_precision = float(min_recall), float(min_precision)
        self.max_boxes, self.capacity_frames = int(max_boxes), int(capacity_frames)
        self._ths = (ctypes.c_float * _lib.EVAL_THRESHOLDS)(*self.dist_ths)
        self.n_frames = 0
        self.frame_ids = []
        self._records = self._gt_count = self._period = self._flags = self._rec_interp = None

    # ---- epoch state --------------------------------------------------------------------------------------------------------------------
    def reset(self):
        self.n_frames = 0
        self.frame_ids = []

    def _buffers(self, device):
        if self._records is None or self._records.device != device:
            C, W = len(self.class_names), _lib.EVAL_RECORD_WORDS
            self._records = torch.zeros((self.capacity_frames * self.max_boxes, W), dtype=torch.int32, device=device)
            self._gt_count = torch.zeros((self.capacity_frames, C), dtype=torch.int32, device=device)
            proto = [class_protocol(n) for n in self.class_names]
            self._period = torch.tensor([p for p, _ in proto], dtype=torch.float32).to(device)
            self._flags = torch.tensor([f for _, f in proto], dtype=torch.int32).to(device)
            self._rec_interp = torch.from_numpy(np.linspace(0, 1, _lib.EVAL_POINTS)).to(device)
        return self._records, self._gt_count

    # ---- per batch ----------------------------------------------------------------------------------------------------------------------
    def _check(self, pred_dicts, gt_boxes):
        """every refusal of add(), on the host and before the first launch"""
        cap = _lib.EVAL_MAX_BOXES
        B = len(pred_dicts)
        if B == 0:
            raise ValueError('add() needs at least one frame')
        if not torch.is_tensor(gt_boxes) or gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] not in (8, 10):
            raise ValueError('gt_boxes of shape %s: the evaluation takes (%d, M, 8 | 10) with the class in the last column'
                             % (tuple(gt_boxes.shape) if torch.is_tensor(gt_boxes) else type(gt_boxes), B))
        width = None
        for b, pd in enumerate(pred_dicts):
            bx, sc, lb = pd['pred_boxes'], pd['pred_scores'], pd['pred_labels']
            for what, t in (('pred_boxes', bx), ('pred_scores', sc), ('pred_labels', lb), ('gt_boxes', gt_boxes)):
                if not t.is_cuda:
                    raise _lib.PcpError('%s of frame %d is a %s tensor: the evaluation reads device tensors (it matches up to %d boxes per frame and '
                                        'class where they lie); no CPU fallback exists' % (what, b, t.device, cap))
            if bx.dtype != torch.float32 or sc.dtype != torch.float32 or gt_boxes.dtype != torch.float32:
                raise ValueError('frame %d: boxes %s, scores %s, gt_boxes %s: the match kernel reads float32 (4-byte) rows of 7 | 9 and 8 | 10 columns'
                                 % (b, bx.dtype, sc.dtype, gt_boxes.dtype))
            if lb.dtype != torch.int64:
                raise ValueError('frame %d: pred_labels are %s, the match kernel reads int64 (8-byte) labels' % (b, lb.dtype))
            if bx.dim() != 2 or bx.shape[1] not in (7, 9) or sc.shape != (bx.shape[0],) or lb.shape != (bx.shape[0],):
                raise ValueError('frame %d: pred_boxes %s, pred_scores %s, pred_labels %s: the evaluation takes (n, 7 | 9), (n,), (n,)'
                                 % (b, tuple(bx.shape), tuple(sc.shape), tuple(lb.shape)))
            if width is not None and bx.shape[1] != width:
                raise ValueError('frame %d has %d-wide boxes, frame 0 %d-wide ones' % (b, bx.shape[1], width))
            width = int(bx.shape[1])
        if self.n_frames + B > self.capacity_frames:
            raise ValueError('%d frames this epoch and %d more: the epoch buffer holds capacity_frames = %d' % (self.n_frames, B, self.capacity_frames))
        C = len(self.class_names)
        # a frame that CAN hold more boxes than a workgroup stages: count per class (a small read, only on this path)
        for b, pd in enumerate(pred_dicts):
            if min(int(pd['pred_boxes'].shape[0]), self.max_boxes) > cap:
                lb = self._top(pd)[2]
                n = torch.bincount(lb.clamp(0, C), minlength=C + 1)[1:].cpu().numpy()
                if n.max() > cap:
                    raise ValueError('frame %d holds %d predictions of class %s: the match kernel takes %d per frame and class'
                                     % (b, int(n.max()), self.class_names[int(n.argmax())], cap))
        if gt_boxes.shape[1] > cap:
            cls = gt_boxes[..., -1].long().clamp(0, C)
            n = torch.stack([torch.bincount(cls[b], minlength=C + 1)[1:] for b in range(B)]).cpu().numpy()
            if n.max() > cap:
                b, c = np.unravel_index(int(n.argmax()), n.shape)
                raise ValueError('frame %d holds %d ground-truth boxes of class %s: the match kernel takes %d per frame and class'
                                 % (b, int(n.max()), self.class_names[c], cap))
        return width

    def _top(self, pd):
        """the frame's detections, cut to the max_boxes best by score"""
        bx, sc, lb = pd['pred_boxes'], pd['pred_scores'], pd['pred_labels']
        if bx.shape[0] > self.max_boxes:
            keep = torch.sort(sc, descending=True, stable=True).indices[:self.max_boxes]
            bx, sc, lb = bx[keep], sc[keep], lb[keep]
        return bx, sc, lb

    def add(self, pred_dicts, gt_boxes, frame_ids=None):
        """pred_dicts: per frame {'pred_boxes' (n, 7 | 9), 'pred_scores' (n,), 'pred_labels' (n,) int64} device tensors; gt_boxes (B, M, 8 | 10)"""
        width = self._check(pred_dicts, gt_boxes)
        B, K, dev = len(pred_dicts), self.max_boxes, gt_boxes.device
        records, gt_count = self._buffers(dev)
        boxes = torch.zeros((B, K, width), dtype=torch.float32, device=dev)
        scores = torch.zeros((B, K), dtype=torch.float32, device=dev)
        labels = torch.zeros((B, K), dtype=torch.int64, device=dev)
        counts = []
        for b, pd in enumerate(pred_dicts):
            bx, sc, lb = self._top(pd)
            n = int(bx.shape[0])
            counts.append(n)
            if n:
                boxes[b, :n], scores[b, :n], labels[b, :n] = bx, sc, lb
        count = torch.tensor(counts, dtype=torch.int32).to(dev)
        gt = gt_boxes.contiguous()
        check(_lib.load().pcp_det_eval_match(_p(boxes), _p(scores), _p(labels), _p(count), B, K, width, _p(gt), int(gt.shape[1]), int(gt.shape[2]),
                                             len(self.class_names), self._ths, self.tp_index, _p(self._period), _p(self._flags), self.n_frames,
                                             _p(records), _p(gt_count), _stream()), 'pcp_det_eval_match')
        self.frame_ids += list(frame_ids) if frame_ids is not None else list(range(self.n_frames, self.n_frames + B))
        self.n_frames += B

    # ---- per epoch ----------------------------------------------------------------------------------------------------------------------
    def records(self):
        """the epoch's records on the host (a read of its own, for inspection and tests): dict of (frames, max_boxes) arrays"""
        K = self.max_boxes
        if self._records is None or self.n_frames == 0:
            raw = np.zeros((0, K, _lib.EVAL_RECORD_WORDS), dtype=np.int32)
        else:
            raw = self._records[:self.n_frames * K].cpu().numpy().reshape(self.n_frames, K, _lib.EVAL_RECORD_WORDS)
        f = np.ascontiguousarray(raw).view(np.float32)
        return {'score': f[..., 0], 'class': raw[..., 1], 'tp_mask': raw[..., 2], 'match': raw[..., 3], 'trans_err': f[..., 4], 'scale_err': f[..., 5],
                'orient_err': f[..., 6], 'vel_err': f[..., 7]}

    def _curves(self):
        """sort, the curve kernel, the one read -> (C, stride) float64"""
        C, L = len(self.class_names), _lib.load()
        stride = int(L.pcp_det_eval_curves_stride())
        if self._records is None:
            raise _lib.PcpError('result() before the first add(): the evaluation has no device yet')
        dev = self._records.device
        N = self.n_frames * self.max_boxes
        rec = self._records[:N]
        score = rec[:, 0].contiguous().view(torch.float32)
        cls = rec[:, 1].contiguous()
        o1 = torch.sort(score, descending=True, stable=True).indices           # ties: the lower (frame, slot) stays in front
        o2 = torch.sort(cls[o1], stable=True).indices
        order = o1[o2]
        srt = rec[order].contiguous()
        class_start = torch.searchsorted(cls[order].contiguous(), torch.arange(C + 2, dtype=torch.int32, device=dev)).to(torch.int32)
        npos = self._gt_count[:self.n_frames].sum(0).to(torch.int32)
        ws_bytes = int(L.pcp_det_eval_curves_workspace_bytes(N))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
        out = torch.empty((C, stride), dtype=torch.float64, device=dev)
        check(L.pcp_det_eval_curves(_p(srt), N, _p(class_start), _p(npos), C, self.tp_index, _p(self._rec_interp), _p(ws), ws_bytes, _p(out),
                                    _stream()), 'pcp_det_eval_curves')
        return out.cpu().numpy()

    def result(self, mean_attr_err=None, version='default'):
        """-> (metrics, text): {'mean_ap', 'label_aps' {class: {d: ap}}, 'label_tp_errors' {class: {metric: err}}, 'mean_dist_aps',
        'tp_errors' {metric: mean over classes}, 'curves', ['nd_score' when mean_attr_err is given]} and the reference's result block"""
        raw = self._curves()
        T, P = _lib.EVAL_THRESHOLDS, _lib.EVAL_POINTS
        first = int(round(100 * self.min_recall)) + 1
        m = {'label_aps': {}, 'label_tp_errors': {}, 'mean_dist_aps': {}, 'curves': {}}
        for c, name in enumerate(self.class_names):
            prec, conf, err = (raw[c, i * T * P:(i + 1) * T * P].reshape(T, P) for i in range(3))
            tail = raw[c, 3 * T * P:]
            m['curves'][name] = {'precision': prec, 'confidence': conf, 'errors': {k: err[i] for i, k in enumerate(METRICS)},
                                 'npos': int(tail[0]), 'ntp': [int(v) for v in tail[1:1 + T]], 'n_pred': int(tail[1 + T])}
            m['label_aps'][name] = {}
            for t, d in enumerate(self.dist_ths):
                p = np.clip(prec[t, first:] - self.min_precision, 0.0, None)
                m['label_aps'][name][d] = float(p.mean() / (1.0 - self.min_precision))
            m['mean_dist_aps'][name] = float(np.mean(list(m['label_aps'][name].values())))
            nz = np.nonzero(conf[self.tp_index] > 0)[0]
            last = int(nz[-1]) if nz.size else -1
            nan_orient, nan_vel = (class_protocol(name)[1] & _lib.EVAL_NAN_ORIENT), (class_protocol(name)[1] & _lib.EVAL_NAN_VEL)
            m['label_tp_errors'][name] = {}
            for i, k in enumerate(METRICS):
                if (k == 'orient_err' and nan_orient) or (k == 'vel_err' and nan_vel):
                    v = float('nan')
                else:
                    v = 1.0 if last < first else float(err[i, first:last + 1].mean())
                m['label_tp_errors'][name][k] = v
        m['mean_ap'] = float(np.mean([ap for name in self.class_names for ap in m['label_aps'][name].values()]))
        m['tp_errors'] = {}
        for k in METRICS:
            vals = np.array([m['label_tp_errors'][name][k] for name in self.class_names], dtype=np.float64)
            m['tp_errors'][k] = float(vals[~np.isnan(vals)].mean()) if (~np.isnan(vals)).any() else float('nan')
        if mean_attr_err is not None:
            five = [m['tp_errors'][k] for k in METRICS] + [float(mean_attr_err)]
            m['nd_score'] = float((5.0 * m['mean_ap'] + sum(1.0 - min(1.0, e) for e in five)) / 10.0)
        return m, format_results(m, self.class_names, version)
