"""The nuScenes detection protocol restated in float64 numpy with plain loops, and a case generator for it.

This file is the reference the device evaluation (pcp_amd/det_eval.py, csrc/det_eval.hip) is tested against; nuscenes-devkit is not
available.  A frame is a dict: 'boxes' (n, 7 | 9) float32 [x y z dx dy dz heading (vx vy)], 'scores' (n,) float32, 'labels' (n,) int64 in
1 .. len(class_names), 'gt' (m, 8 | 10) float32 with the class in the last column (0 = padding row).

evaluate() walks ALL predictions of a class over ALL frames by descending score (python's stable sort: ties keep (frame, index) order) with
one taken-set per frame, and forms the curves with numpy.interp.
"""
import numpy as np

DIST_THS = (0.5, 1.0, 2.0, 4.0)
METRICS = ('trans_err', 'scale_err', 'orient_err', 'vel_err')
NUSC_CLASSES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']


def angle_diff(x, y, period):
    d = (x - y + period / 2) % period - period / 2
    if d > np.pi:
        d = d - 2 * np.pi
    return d


def nan_metrics(name):
    """the (class, metric) pairs the protocol does not measure"""
    if name == 'traffic_cone':
        return ('orient_err', 'vel_err')
    if name == 'barrier':
        return ('vel_err',)
    return ()


def pair_errors(pred, gt_row, name):
    """float64 errors of a matched pair; pred (7 | 9,), gt_row (8 | 10,)"""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt_row, dtype=np.float64)
    trans = float(np.sqrt((p[0] - g[0]) ** 2 + (p[1] - g[1]) ** 2))
    inter = min(p[3], g[3]) * min(p[4], g[4]) * min(p[5], g[5])
    va, vb = g[3] * g[4] * g[5], p[3] * p[4] * p[5]
    scale = 1.0 - inter / (va + vb - inter)
    period = np.pi if name == 'barrier' else 2 * np.pi
    orient = abs(angle_diff(g[6], p[6], period))
    vel = 0.0
    if p.shape[0] == 9 and g.shape[0] == 10:
        vel = float(np.sqrt((g[7] - p[7]) ** 2 + (g[8] - p[8]) ** 2))
    out = {'trans_err': trans, 'scale_err': float(scale), 'orient_err': float(orient), 'vel_err': vel}
    for m in nan_metrics(name):
        out[m] = float('nan')
    return out


def cummean(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).sum() == len(x):
        return np.ones(len(x))
    s = np.nancumsum(x)
    c = np.cumsum(~np.isnan(x))
    return np.divide(s, c, out=np.zeros_like(s), where=c != 0)


def no_predictions():
    return {'precision': np.zeros(101), 'confidence': np.zeros(101), 'errors': {m: np.ones(101) for m in METRICS}}


def accumulate(frames, cls_id, name, dist_th, with_errors, record_errors=None):
    """-> curve data of one (class, threshold), per-prediction TP flags / matched rows keyed (frame, index).  record_errors: optional
    {(frame, index): {metric: value}} used INSTEAD of the float64 pair errors (to feed the curves the device's float32 errors)"""
    npos = sum(int((np.asarray(f['gt'])[:, -1] == cls_id).sum()) if len(f['gt']) else 0 for f in frames)
    preds = [(float(f['scores'][i]), fi, i) for fi, f in enumerate(frames) for i in range(len(f['scores'])) if int(f['labels'][i]) == cls_id]
    flags, match = {}, {}
    out = no_predictions()
    out.update(npos=npos, ntp=0)
    if npos == 0 or not preds:
        for _, fi, i in preds:
            flags[(fi, i)], match[(fi, i)] = 0, -1
        return out, flags, match, {}
    preds.sort(key=lambda r: -r[0])
    taken = [set() for _ in frames]
    tp, fp, conf, errs, tp_conf, pair = [], [], [], {m: [] for m in METRICS}, [], {}
    for score, fi, i in preds:
        f = frames[fi]
        best, best_j = np.inf, -1
        for j in range(len(f['gt'])):
            if f['gt'][j, -1] != cls_id or j in taken[fi]:
                continue
            d = np.sqrt((np.float64(f['boxes'][i, 0]) - np.float64(f['gt'][j, 0])) ** 2 + (np.float64(f['boxes'][i, 1]) - np.float64(f['gt'][j, 1])) ** 2)
            if d < best:
                best, best_j = d, j
        hit = best < dist_th
        conf.append(score)
        tp.append(1 if hit else 0)
        fp.append(0 if hit else 1)
        flags[(fi, i)], match[(fi, i)] = int(hit), (best_j if hit else -1)
        if hit:
            taken[fi].add(best_j)
            e = pair_errors(f['boxes'][i], f['gt'][best_j], name)
            pair[(fi, i)] = e
            if record_errors is not None:
                e = record_errors[(fi, i)]
            tp_conf.append(score)
            for m in METRICS:
                errs[m].append(e[m])
    tp_c, fp_c, conf = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float), np.array(conf, dtype=np.float64)
    prec, rec = tp_c / (fp_c + tp_c), tp_c / float(npos)
    rec_interp = np.linspace(0, 1, 101)
    out['precision'] = np.interp(rec_interp, rec, prec, right=0)
    out['confidence'] = np.interp(rec_interp, rec, conf, right=0)
    out['ntp'] = int(sum(tp))
    if with_errors and tp_conf:
        tc = np.array(tp_conf, dtype=np.float64)
        for m in METRICS:
            out['errors'][m] = np.interp(out['confidence'][::-1], tc[::-1], cummean(errs[m])[::-1])[::-1]
    return out, flags, match, pair


def calc_ap(precision, min_recall, min_precision):
    prec = np.copy(precision)[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(confidence, curve, min_recall):
    first = round(100 * min_recall) + 1
    nz = np.nonzero(confidence)[0]
    last = int(nz[-1]) if len(nz) else -1
    if last < first:
        return 1.0
    return float(np.mean(curve[first:last + 1]))


def evaluate(frames, class_names, dist_ths=DIST_THS, dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, mean_attr_err=None, record_errors=None):
    """-> dict: 'curves' {name: {'precision' (T, 101), 'confidence' (T, 101), 'errors' {metric: (101,)}, 'npos', 'ntp' [T]}},
    'tp_mask' / 'match' {(frame, index): bits / gt row at dist_th_tp}, 'pair_errors' {(frame, index): {metric: float64}}, and the summary
    values 'label_aps', 'label_tp_errors', 'mean_dist_aps', 'mean_ap', 'tp_errors' (and 'nd_score' with mean_attr_err)"""
    res = {'curves': {}, 'tp_mask': {}, 'match': {}, 'pair_errors': {}, 'label_aps': {}, 'label_tp_errors': {}, 'mean_dist_aps': {}}
    for ci, name in enumerate(class_names):
        cur = {'precision': [], 'confidence': [], 'ntp': []}
        res['label_aps'][name] = {}
        for t, d in enumerate(dist_ths):
            is_tp = d == dist_th_tp
            data, flags, match, pair = accumulate(frames, ci + 1, name, d, is_tp, record_errors)
            cur['precision'].append(data['precision'])
            cur['confidence'].append(data['confidence'])
            cur['ntp'].append(data['ntp'])
            cur['npos'] = data['npos']
            for key, v in flags.items():
                res['tp_mask'][key] = res['tp_mask'].get(key, 0) | (v << t)
            if is_tp:
                cur['errors'] = data['errors']
                res['match'].update(match)
                res['pair_errors'].update(pair)
                res['label_tp_errors'][name] = {}
                for m in METRICS:
                    res['label_tp_errors'][name][m] = float('nan') if m in nan_metrics(name) else calc_tp(data['confidence'], data['errors'][m], min_recall)
            res['label_aps'][name][d] = calc_ap(data['precision'], min_recall, min_precision)
        cur['precision'], cur['confidence'] = np.stack(cur['precision']), np.stack(cur['confidence'])
        res['curves'][name] = cur
        res['mean_dist_aps'][name] = float(np.mean(list(res['label_aps'][name].values())))
    res['mean_ap'] = float(np.mean([ap for name in class_names for ap in res['label_aps'][name].values()]))
    res['tp_errors'] = {}
    for m in METRICS:
        vals = np.array([res['label_tp_errors'][name][m] for name in class_names], dtype=np.float64)
        res['tp_errors'][m] = float(np.nanmean(vals)) if (~np.isnan(vals)).any() else float('nan')
    if mean_attr_err is not None:
        five = [res['tp_errors'][m] for m in METRICS] + [float(mean_attr_err)]
        res['nd_score'] = float((5.0 * res['mean_ap'] + sum(1.0 - min(1.0, e) for e in five)) / 10.0)
    return res


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _random_box(rng, xy, width):
    row = np.zeros(width, dtype=np.float32)
    row[0:2] = xy
    row[2] = rng.uniform(-2.0, 0.0)
    row[3:6] = rng.uniform(0.5, 5.0, 3)
    row[6] = rng.uniform(-np.pi, np.pi)
    if width >= 9:
        row[7:9] = rng.uniform(-6.0, 6.0, 2)
    return row


def check_conditioning(frames, dist_ths=DIST_THS, eps=1e-3, distinct_scores=True):
    """the conditions under which float32 arithmetic cannot flip a match against float64"""
    if distinct_scores:
        s = np.concatenate([np.asarray(f['scores'], dtype=np.float32) for f in frames]) if frames else np.zeros(0, np.float32)
        assert len(np.unique(s)) == len(s), 'scores are not distinct'
    reach = max(dist_ths) + eps
    for f in frames:
        for i in range(len(f['scores'])):
            rows = np.nonzero(f['gt'][:, -1] == f['labels'][i])[0] if len(f['gt']) else np.zeros(0, int)
            if not len(rows):
                continue
            d = np.sqrt(((f['gt'][rows, :2].astype(np.float64) - f['boxes'][i, :2].astype(np.float64)) ** 2).sum(1))
            for th in dist_ths:
                assert np.abs(d - th).min() >= eps, 'a distance within %g of the threshold %g' % (eps, th)
            d = np.sort(d)
            if len(d) > 1:
                assert d[1] - d[0] >= eps, 'the two nearest ground-truth rows are %g apart in distance' % (d[1] - d[0])
                near = d[d < reach]                          # any two rows a prediction could still take must be told apart too
                assert len(near) < 2 or np.diff(near).min() >= eps
    return True


def make_case(seed, n_pred, n_gt, class_names, box_width=7, gt_width=8, max_pad=None, half=50.0, class_weights=None, gt_weights=None, dist_ths=DIST_THS):
    """n_pred / n_gt: per frame counts (lists of equal length).  Most predictions sit at a drawn distance from a ground-truth row of their
    class (every band between the thresholds is hit), the rest anywhere.  gt rows are zero-padded to max(n_gt) (or max_pad) rows.  Every
    prediction is redrawn until check_conditioning's conditions hold for it."""
    rng = np.random.RandomState(seed)
    C = len(class_names)
    total = int(sum(n_pred))
    scores = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)
    assert len(np.unique(scores)) == total
    bands = [(0.05, 0.45), (0.55, 0.95), (1.05, 1.95), (2.05, 3.95), (4.05, 9.0)]
    M = max(max(n_gt), 1) if max_pad is None else max_pad
    frames, s0 = [], 0
    w = np.ones(C) / C if class_weights is None else np.asarray(class_weights, dtype=np.float64) / np.sum(class_weights)
    wg = w if gt_weights is None else np.asarray(gt_weights, dtype=np.float64) / np.sum(gt_weights)      # a class may have no ground truth at all
    for npd, ng in zip(n_pred, n_gt):
        gt = np.zeros((M, gt_width), dtype=np.float32)
        for j in range(ng):
            gt[j, :gt_width - 1] = _random_box(rng, rng.uniform(-half, half, 2), gt_width - 1)
            gt[j, -1] = 1 + rng.choice(C, p=wg)
        boxes = np.zeros((npd, box_width), dtype=np.float32)
        labels = np.zeros(npd, dtype=np.int64)
        for i in range(npd):
            for _ in range(1000):
                labels[i] = 1 + rng.choice(C, p=w)
                rows = np.nonzero(gt[:, -1] == labels[i])[0]
                if len(rows) and rng.uniform() < 0.8:
                    lo, hi = bands[rng.randint(len(bands))]
                    r, a = rng.uniform(lo, hi), rng.uniform(-np.pi, np.pi)
                    xy = gt[rng.choice(rows), :2] + np.array([r * np.cos(a), r * np.sin(a)])
                else:
                    xy = rng.uniform(-half, half, 2)
                boxes[i] = _random_box(rng, xy, box_width)
                if len(rows) and rng.uniform() < 0.5:         # near-copies of the matched box: small but non-zero scale / heading errors
                    g = gt[rows[np.argmin(((gt[rows, :2] - boxes[i, :2]) ** 2).sum(1))]]
                    boxes[i, 3:6] = g[3:6] * rng.uniform(0.8, 1.25, 3).astype(np.float32)
                    boxes[i, 6] = g[6] + rng.uniform(-0.5, 0.5)
                one = {'boxes': boxes[i:i + 1], 'scores': scores[s0 + i:s0 + i + 1], 'labels': labels[i:i + 1], 'gt': gt}
                try:
                    check_conditioning([one], dist_ths, distinct_scores=False)
                    break
                except AssertionError:
                    continue
            else:
                raise AssertionError('no well-conditioned prediction found')
        frames.append({'boxes': boxes, 'scores': scores[s0:s0 + npd].copy(), 'labels': labels, 'gt': gt})
        s0 += npd
    check_conditioning(frames, dist_ths)
    return frames


def tie_case():
    """equal scores and equidistant ground truth: the lower prediction index goes first, the lower row wins.  One class, two frames."""
    def box(x, y):
        return [x, y, -1.0, 4.0, 2.0, 1.5, 0.0]
    gt0 = np.array([box(0, 0) + [1], box(3, 0) + [1], box(10, 10) + [1], box(13, 10) + [1]], dtype=np.float32)
    b0 = np.array([box(0.25, 0), box(-0.25, 0), box(11.5, 10), box(11.5, 10.25)], dtype=np.float32)
    s0 = np.array([0.9, 0.9, 0.5, 0.5], dtype=np.float32)
    gt1 = np.array([box(20, 20) + [1], box(-20, -20) + [1]], dtype=np.float32)
    b1 = np.array([box(20, 23), box(-20, -20.25)], dtype=np.float32)          # the first is a miss up to 2 m, the second a hit, same score as frame 0's
    s1 = np.array([0.9, 0.9], dtype=np.float32)
    gt1 = np.concatenate([gt1, np.zeros((2, 8), np.float32)])
    return [{'boxes': b0, 'scores': s0, 'labels': np.ones(4, np.int64), 'gt': gt0}, {'boxes': b1, 'scores': s1, 'labels': np.ones(2, np.int64), 'gt': gt1}]
