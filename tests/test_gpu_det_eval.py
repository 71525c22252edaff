"""pcp_amd/det_eval.py + csrc/det_eval.hip against the float64 restatement of the protocol (tests/det_eval_refs.py) on the same float32
inputs.  The generated cases are conditioned (distinct scores, no distance within 1e-3 of a threshold, candidate rows at least 1e-3 apart in
distance) so that float32 against float64 cannot flip a match: masks, matched rows and counts must be EQUAL, the float64 curve arithmetic
within 1e-9.

Per-record errors are float32 on the device: bound 3.05e-5 (4 ulp at 64 m).  The error CURVES are running means of those float32 values, so
against the float64 restatement they differ by as much as the records do -- measured maximum over the cases below 4.14e-7 (curves) and
3.59e-7 (TP means), bounded here by ten times that; fed the device's own float32 errors, the restatement must give the same curves to 1e-9."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import det_eval_refs as R

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
RECORD_TOL = 3.05e-5
F64_TOL = 1e-9
ERR_CURVE_TOL = 4.14e-6         # ten times the measured 4.14e-7 (see the module docstring)
MINI_RANGE = [-12.8, -12.8, -8.0, 12.8, 12.8, 0.0]


def _device(frames):
    pds = [{'pred_boxes': torch.from_numpy(f['boxes']).cuda(), 'pred_scores': torch.from_numpy(f['scores']).cuda(),
            'pred_labels': torch.from_numpy(f['labels']).cuda()} for f in frames]
    return pds, torch.from_numpy(np.stack([f['gt'] for f in frames])).cuda()


def _evaluator(names, frames, max_boxes, splits=None):
    from pcp_amd.det_eval import DeviceDetectionEval
    ev = DeviceDetectionEval(names, max_boxes=max_boxes, capacity_frames=len(frames))
    pds, gt = _device(frames)
    for lo, hi in (splits or [(0, len(frames))]):
        ev.add(pds[lo:hi], gt[lo:hi])
    return ev


def _maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), 'NaNs in different places'
    return float(np.nanmax(np.abs(a - b))) if a.size and (~np.isnan(a)).any() else 0.0


def _check(names, frames, max_boxes):
    ev = _evaluator(names, frames, max_boxes)
    ref = R.evaluate(frames, names)
    rec = ev.records()
    worst_rec, dev_errors = 0.0, {}
    for fi, f in enumerate(frames):
        n = len(f['scores'])
        assert np.array_equal(rec['class'][fi, :n], f['labels']) and (rec['class'][fi, n:] == 0).all()
        assert np.array_equal(rec['score'][fi, :n], f['scores'])
        for i in range(n):
            assert rec['tp_mask'][fi, i] == ref['tp_mask'][(fi, i)], (fi, i, rec['tp_mask'][fi, i], ref['tp_mask'][(fi, i)])
            assert rec['match'][fi, i] == ref['match'][(fi, i)], (fi, i)
            dev_errors[(fi, i)] = {m: float(rec[m][fi, i]) for m in R.METRICS}
            if (fi, i) in ref['pair_errors']:
                worst_rec = max(worst_rec, _maxdiff([rec[m][fi, i] for m in R.METRICS], [ref['pair_errors'][(fi, i)][m] for m in R.METRICS]))
            else:
                assert all(rec[m][fi, i] == 0.0 for m in R.METRICS)
    metrics, text = ev.result()
    own = R.evaluate(frames, names, record_errors=dev_errors)           # the restatement on the device's float32 errors
    worst = {'pr': 0.0, 'curve64': 0.0, 'curve_own': 0.0, 'ap': 0.0, 'tp64': 0.0, 'tp_own': 0.0}
    for name in names:
        got, want = metrics['curves'][name], ref['curves'][name]
        assert got['npos'] == want['npos'] and got['ntp'] == want['ntp'], (name, got['npos'], want['npos'], got['ntp'], want['ntp'])
        worst['pr'] = max(worst['pr'], _maxdiff(got['precision'], want['precision']), _maxdiff(got['confidence'], want['confidence']))
        for m in R.METRICS:
            worst['curve64'] = max(worst['curve64'], _maxdiff(got['errors'][m], want['errors'][m]))
            worst['curve_own'] = max(worst['curve_own'], _maxdiff(got['errors'][m], own['curves'][name]['errors'][m]))
            worst['tp64'] = max(worst['tp64'], _maxdiff(metrics['label_tp_errors'][name][m], ref['label_tp_errors'][name][m]))
            worst['tp_own'] = max(worst['tp_own'], _maxdiff(metrics['label_tp_errors'][name][m], own['label_tp_errors'][name][m]))
        for d in R.DIST_THS:
            worst['ap'] = max(worst['ap'], abs(metrics['label_aps'][name][d] - ref['label_aps'][name][d]))
    for m in R.METRICS:
        worst['tp64'] = max(worst['tp64'], _maxdiff(metrics['tp_errors'][m], ref['tp_errors'][m]))
    worst['ap'] = max(worst['ap'], abs(metrics['mean_ap'] - ref['mean_ap']))
    print('det_eval figures: record errors %.3g, precision/confidence %.3g, AP %.3g, error curves vs float64 %.3g, vs own float32 errors %.3g, '
          'TP means vs float64 %.3g, vs own %.3g' % (worst_rec, worst['pr'], worst['ap'], worst['curve64'], worst['curve_own'], worst['tp64'],
                                                     worst['tp_own']))
    assert worst_rec <= RECORD_TOL
    assert worst['pr'] <= F64_TOL and worst['ap'] <= F64_TOL
    assert worst['curve_own'] <= F64_TOL and worst['tp_own'] <= F64_TOL
    assert worst['curve64'] <= ERR_CURVE_TOL and worst['tp64'] <= ERR_CURVE_TOL
    assert 'mAP:\t %.4f' % ref['mean_ap'] in text
    return ev, metrics, ref


def test_mixed_small_case():
    """B = 3, K = 64, M = 20, 7- and 8-wide: a frame without predictions, a frame without ground truth, a class without ground truth
    anywhere, more predictions than ground truth"""
    names = ['car', 'pedestrian']
    frames = R.make_case(11, [64, 0, 40], [12, 9, 0], names, max_pad=20, gt_weights=[1, 0])
    _ev, metrics, ref = _check(names, frames, 64)
    assert metrics['curves']['pedestrian']['npos'] == 0 and metrics['label_aps']['pedestrian'][2.0] == 0.0
    assert 0.0 < ref['label_aps']['car'][4.0] < 1.0


def test_capacity_case():
    """one frame at the capacity: 512 predictions (the sort at full width) and 130 ground-truth rows of one class (three passes of a wave)"""
    frames = R.make_case(12, [512], [130], ['car'])
    _ev, metrics, _ref = _check(['car'], frames, 512)
    assert metrics['curves']['car']['n_pred'] == 512 and metrics['curves']['car']['npos'] == 130


def test_ten_class_case():
    """the nuScenes names, 9-wide predictions against 10-wide ground truth: velocity error, the barrier period, the traffic-cone NaNs"""
    frames = R.make_case(13, [60, 60], [40, 40], R.NUSC_CLASSES, box_width=9, gt_width=10)
    ev, metrics, _ref = _check(R.NUSC_CLASSES, frames, 64)
    e = metrics['label_tp_errors']
    assert np.isnan(e['traffic_cone']['orient_err']) and np.isnan(e['traffic_cone']['vel_err']) and np.isnan(e['barrier']['vel_err'])
    assert np.isfinite(e['barrier']['orient_err']) and np.isfinite(e['car']['vel_err'])
    rec = ev.records()
    cone = rec['class'] == 1 + R.NUSC_CLASSES.index('traffic_cone')
    hit = cone & (rec['match'] >= 0)
    assert hit.any() and np.isnan(rec['orient_err'][hit]).all() and np.isnan(rec['vel_err'][hit]).all()
    assert (rec['vel_err'][(rec['class'] == 1) & (rec['match'] >= 0)] > 0).any()


def test_tie_case():
    """equal scores, and predictions equidistant from two rows: the lower prediction slot goes first, the lower row is taken, and the epoch
    order puts the lower frame first"""
    frames = R.tie_case()
    ev, _metrics, _ref = _check(['car'], frames, 8)
    rec = ev.records()
    assert list(rec['tp_mask'][0, :4]) == [15, 8, 12, 12] and list(rec['match'][0, :4]) == [0, -1, 2, 3]
    assert list(rec['tp_mask'][1, :2]) == [8, 15]


def test_split_epochs_and_repeated_results_are_bit_equal():
    names = ['car', 'pedestrian']
    frames = R.make_case(11, [64, 0, 40], [12, 9, 0], names, max_pad=20, gt_weights=[1, 0])
    one = _evaluator(names, frames, 64)
    three = _evaluator(names, frames, 64, splits=[(0, 1), (1, 2), (2, 3)])
    a, b = one._curves(), three._curves()
    assert a.tobytes() == b.tobytes()
    assert one._curves().tobytes() == a.tobytes()
    ra, rb = one.records(), three.records()
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra)
    one.reset()
    one.add(*_device(frames[2:]))
    assert one.n_frames == 1 and one.result()[0]['curves']['car']['npos'] == 0


def test_refusals_come_before_any_launch():
    from pcp_amd.det_eval import DeviceDetectionEval
    from pcp_amd.lib import PcpError
    ev = DeviceDetectionEval(['car', 'pedestrian'], max_boxes=600, capacity_frames=2)
    n = 520
    pd = {'pred_boxes': torch.zeros(n, 7).cuda(), 'pred_scores': torch.rand(n).cuda(), 'pred_labels': torch.ones(n, dtype=torch.int64).cuda()}
    pd['pred_labels'][513:] = 2
    gt = torch.zeros(1, 4, 8).cuda()
    with pytest.raises(ValueError, match=r'513 predictions of class car.*512'):
        ev.add([pd], gt)
    ok = {k: v[:8] for k, v in pd.items()}
    with pytest.raises(PcpError, match='512'):
        ev.add([{k: v.cpu() for k, v in ok.items()}], gt)
    with pytest.raises(PcpError, match='512'):
        ev.add([ok], gt.cpu())
    with pytest.raises(ValueError, match=r'float64.*float32 \(4-byte\)'):
        ev.add([dict(ok, pred_boxes=ok['pred_boxes'].double())], gt)
    with pytest.raises(ValueError, match='capacity_frames = 2'):
        ev.add([ok, ok, ok], torch.zeros(3, 4, 8).cuda())
    gt_many = torch.zeros(1, 600, 8).cuda()
    gt_many[0, :515, 7] = 2
    with pytest.raises(ValueError, match=r'515 ground-truth boxes of class pedestrian.*512'):
        ev.add([ok], gt_many)
    assert ev.n_frames == 0 and (ev._records is None or int(ev._records.abs().sum()) == 0)
    ev.add([ok], gt)                                                   # and the evaluator still works afterwards
    assert ev.n_frames == 1


def _run_test_py(extra):
    tools = os.path.join(REPO, 'practical-collab-perception_amd', 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', 'cfgs/v2x_sim_models/v2x_pointpillar_basic_ego.yaml', '--batch_size', '2'] + extra + \
          ['--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE), 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '3000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '3', 'DATA_CONFIG.SYNTHETIC.EVAL_GT', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    return r.stdout + r.stderr


@pytest.mark.parametrize('fast', [False, True])
def test_tools_test_py_device_eval_reports_map(fast):
    """tools/test.py --device_eval at a mini range with SYNTHETIC.EVAL_GT, the batch-by-batch loop and the pipelined one"""
    out = _run_test_py(['--device_eval'] + (['--fast'] if fast else []))
    assert 'Nuscene default results' in out and re.search(r'mAP:\t \d\.\d{4}', out), out[-1500:]
    m = re.search(r'mean_ap ([0-9.eE+-]+) over (\d+) detections, (\d+) frames', out)
    assert m is not None and np.isfinite(float(m.group(1))) and 0.0 <= float(m.group(1)) <= 1.0 and int(m.group(3)) == 3, out[-1500:]
    assert 'no ground truth, no mAP' not in out


def test_tools_test_py_without_the_flag_reports_the_old_line():
    out = _run_test_py([])
    assert re.search(r'synthetic data: \d+ detections over 3 frames \(no ground truth, no mAP\)', out), out[-1500:]
    assert 'Nuscene default results' not in out
