"""The float64 restatement of the nuScenes detection protocol (tests/det_eval_refs.py) checked on its own, and the host-only parts of the
device evaluation (pcp_amd/det_eval.py, the dataset option, the formatter): no GPU."""
import os

import numpy as np
import pytest
import torch

import det_eval_refs as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _box(x, y, yaw=0.0, size=(4.0, 2.0, 1.5), vel=None):
    row = [x, y, -1.0, size[0], size[1], size[2], yaw]
    return row + list(vel) if vel is not None else row


def _frame(boxes, scores, labels, gt):
    return {'boxes': np.asarray(boxes, dtype=np.float32).reshape(len(scores), -1), 'scores': np.asarray(scores, dtype=np.float32),
            'labels': np.asarray(labels, dtype=np.int64), 'gt': np.asarray(gt, dtype=np.float32)}


def test_predictions_equal_to_the_ground_truth_score_one():
    rng = np.random.RandomState(3)
    names = ['car', 'pedestrian']
    frames = []
    for _ in range(3):
        gt = np.zeros((12, 8), dtype=np.float32)
        for j in range(10):
            gt[j, :7] = R._random_box(rng, rng.uniform(-40, 40, 2), 7)
            gt[j, 7] = 1 + j % 2
        frames.append(_frame(gt[:10, :7], rng.permutation(10) / 10.0 + 0.05 + 0.01 * len(frames), gt[:10, 7], gt))
    res = R.evaluate(frames, names)
    for name in names:
        for d in R.DIST_THS:
            assert abs(res['label_aps'][name][d] - 1.0) < 1e-12
        for m in R.METRICS:
            assert res['label_tp_errors'][name][m] == 0.0
    assert abs(res['mean_ap'] - 1.0) < 1e-12 and all(v == 0.0 for v in res['tp_errors'].values())
    assert all(v == 15 for v in res['tp_mask'].values())


def test_predictions_farther_than_every_threshold_score_zero():
    gt = [_box(0, 0) + [1], _box(20, 0) + [1]]
    frames = [_frame([_box(0, 4.5), _box(20, -5.0), _box(-30, 30)], [0.9, 0.8, 0.7], [1, 1, 1], gt)]
    res = R.evaluate(frames, ['car'], mean_attr_err=1.0)
    assert res['mean_ap'] == 0.0 and all(v == 1.0 for v in res['tp_errors'].values())
    assert all(v == 0 for v in res['tp_mask'].values()) and all(v == -1 for v in res['match'].values())
    assert res['nd_score'] == 0.0
    assert 'nd_score' not in R.evaluate(frames, ['car'])


def test_three_predictions_two_ground_truths_by_hand():
    """p0 (0.9) lies 0.3 m from g0, p1 (0.8) 1.5 m from g1, p2 (0.7) nowhere.  At 0.5 and 1 m: TP FP FP, recall stays 0.5, so the precision
    curve is 1 below recall 0.5, the LAST sample's 1/3 at exactly 0.5 and 0 above.  At 2 and 4 m: TP TP FP, precision 1 below recall 1 and
    the last sample's 2/3 at 1."""
    assert np.linspace(0, 1, 101)[50] == 0.5
    gt = [_box(0, 0) + [1], _box(10, 0) + [1]]
    frames = [_frame([_box(0.3, 0), _box(10, 1.5), _box(20, 20)], [0.9, 0.8, 0.7], [1, 1, 1], gt)]
    res = R.evaluate(frames, ['car'])
    low = (39 * 0.9 + (1.0 / 3.0 - 0.1)) / 90.0 / 0.9                      # recall points 11 .. 49, the point 50, then zeros
    high = (89 * 0.9 + (2.0 / 3.0 - 0.1)) / 90.0 / 0.9                     # recall points 11 .. 99, the point 100
    want = {0.5: low, 1.0: low, 2.0: high, 4.0: high}
    for d in R.DIST_THS:
        assert abs(res['label_aps']['car'][d] - want[d]) < 1e-12, d
    assert res['tp_mask'] == {(0, 0): 15, (0, 1): 12, (0, 2): 0} and res['match'] == {(0, 0): 0, (0, 1): 1, (0, 2): -1}
    assert abs(res['mean_ap'] - (low + high) / 2) < 1e-12
    # trans_err: confidence is 0.9 up to recall 0.5 and falls towards 0.8 below recall 1; AT recall 1 it is the last sample's 0.7, under
    # every match, where the curve holds its end value.  The running means are 0.3 and 0.9; points 11 .. 100
    conf = res['curves']['car']['confidence'][2]
    assert conf[0] == np.float32(0.9) and conf[100] == np.float32(0.7) and conf[99] > np.float32(0.8)
    c9, c8 = float(np.float32(0.9)), float(np.float32(0.8))
    by_hand = np.mean([0.3 + (0.9 - 0.3) * (c9 - c) / (c9 - c8) for c in conf[11:100]] + [0.9])
    assert abs(res['label_tp_errors']['car']['trans_err'] - by_hand) < 1e-6    # the 0.3 / 1.5 m offsets are float32 values
    assert res['curves']['car']['npos'] == 2 and res['curves']['car']['ntp'] == [1, 1, 2, 2]


def test_barrier_period_and_traffic_cone_nans():
    g = np.array(_box(0, 0, yaw=0.0, vel=(1.0, 0.0)) + [1], dtype=np.float32)
    p = np.array(_box(0.1, 0, yaw=np.pi - 0.1, vel=(0.0, 0.0)), dtype=np.float32)
    assert abs(R.pair_errors(p, g, 'car')['orient_err'] - (np.pi - 0.1)) < 1e-6
    assert abs(R.pair_errors(p, g, 'barrier')['orient_err'] - 0.1) < 1e-6
    assert abs(R.pair_errors(p, g, 'car')['vel_err'] - 1.0) < 1e-12 and R.pair_errors(p[:7], g, 'car')['vel_err'] == 0.0
    assert np.isnan(R.pair_errors(p, g, 'barrier')['vel_err'])
    cone = R.pair_errors(p, g, 'traffic_cone')
    assert np.isnan(cone['orient_err']) and np.isnan(cone['vel_err']) and cone['trans_err'] > 0
    assert abs(R.angle_diff(3.0, -3.0, 2 * np.pi) - (6.0 - 2 * np.pi)) < 1e-12
    names = ['barrier', 'traffic_cone', 'car']
    gt = [list(g[:9]) + [c] for c in (1, 2, 3)]
    for j, row in enumerate(gt):
        row[0] = 20.0 * j
    boxes = [list(p) for _ in range(3)]
    for j, row in enumerate(boxes):
        row[0] = 20.0 * j + 0.1
    res = R.evaluate([_frame(boxes, [0.9, 0.8, 0.7], [1, 2, 3], gt)], names)
    e = res['label_tp_errors']
    assert np.isnan(e['barrier']['vel_err']) and not np.isnan(e['barrier']['orient_err'])
    assert np.isnan(e['traffic_cone']['vel_err']) and np.isnan(e['traffic_cone']['orient_err'])
    assert abs(e['barrier']['orient_err'] - 0.1) < 1e-6 and abs(e['car']['orient_err'] - (np.pi - 0.1)) < 1e-6
    assert abs(res['tp_errors']['vel_err'] - 1.0) < 1e-6                                  # the nan-mean: car alone
    assert abs(res['tp_errors']['orient_err'] - (np.pi / 2)) < 1e-6                       # barrier and car
    # the product's class table says the same
    from pcp_amd import det_eval, lib
    for name in R.NUSC_CLASSES:
        period, flags = det_eval.class_protocol(name)
        assert period == (np.pi if name == 'barrier' else 2 * np.pi)
        assert bool(flags & lib.EVAL_NAN_ORIENT) == ('orient_err' in R.nan_metrics(name))
        assert bool(flags & lib.EVAL_NAN_VEL) == ('vel_err' in R.nan_metrics(name))


def test_generated_cases_are_well_conditioned():
    frames = R.make_case(5, [40, 0, 25], [12, 9, 0], ['car', 'pedestrian'], max_pad=20)
    assert R.check_conditioning(frames) and [len(f['scores']) for f in frames] == [40, 0, 25] and frames[0]['gt'].shape == (20, 8)
    frames = R.make_case(6, [30], [25], R.NUSC_CLASSES, box_width=9, gt_width=10)
    assert R.check_conditioning(frames) and frames[0]['boxes'].shape == (30, 9) and frames[0]['gt'].shape[1] == 10
    res = R.evaluate(frames, R.NUSC_CLASSES)
    assert 0.0 < res['mean_ap'] < 1.0
    bad = [_frame([_box(0.5005, 0)], [0.5], [1], [_box(0, 0) + [1]])]
    with pytest.raises(AssertionError):
        R.check_conditioning(bad)
    twin = [_frame([_box(1.5, 0)], [0.5], [1], [_box(0, 0) + [1], _box(3, 0) + [1]])]
    with pytest.raises(AssertionError):
        R.check_conditioning(twin)
    with pytest.raises(AssertionError):
        R.check_conditioning(R.tie_case())                                               # the tie case is the one exception, on purpose
    tie = R.evaluate(R.tie_case(), ['car'])
    assert tie['tp_mask'][(0, 0)] == 15 and tie['tp_mask'][(0, 1)] == 8 and tie['match'][(0, 2)] == 2 and tie['match'][(0, 3)] == 3


def test_formatter_layout_and_host_refusals():
    from pcp_amd import det_eval
    from pcp_amd.lib import PcpError
    frames = R.make_case(8, [20], [10], ['car', 'pedestrian'])
    res = R.evaluate(frames, ['car', 'pedestrian'], mean_attr_err=1.0)
    text = det_eval.format_results(res, ['car', 'pedestrian'])
    lines = text.splitlines()
    assert lines[0] == '----------------Nuscene default results-----------------'
    assert lines[1] == '***car error@trans, scale, orient, vel | AP@0.5, 1.0, 2.0, 4.0'
    assert lines[2].count('|') == 2 and lines[2].endswith('mean AP: %s' % res['mean_dist_aps']['car'])
    assert lines[5] == '--------------average performance-------------'
    assert lines[6] == 'trans_err:\t %.4f' % res['tp_errors']['trans_err']
    assert lines[-2] == 'mAP:\t %.4f' % res['mean_ap'] and lines[-1] == 'NDS:\t %.4f' % res['nd_score']
    ev = det_eval.DeviceDetectionEval(['car', 'pedestrian'], max_boxes=64)
    pd = [{'pred_boxes': torch.zeros(3, 7), 'pred_scores': torch.zeros(3), 'pred_labels': torch.ones(3, dtype=torch.int64)}]
    with pytest.raises(PcpError, match='512'):
        ev.add(pd, torch.zeros(1, 4, 8))                                                 # host tensors: refused before anything is launched
    with pytest.raises(ValueError, match='dist_th_tp'):
        det_eval.DeviceDetectionEval(['car'], dist_th_tp=3.0)
    with pytest.raises(ValueError, match='exactly 4'):
        det_eval.DeviceDetectionEval(['car'], dist_ths=(1, 2))


def test_dataset_option_leaves_evaluation_items_alone_by_default():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    cfg = cfg_from_yaml_file(os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models', 'v2x_pointpillar_basic_ego.yaml'),
                             EasyDict())
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=200, NUM_FRAMES=3)
    ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=False)
    assert sorted(ds[1].keys()) == ['frame_id', 'metadata', 'points']
    assert sorted(next(iter(loader)).keys()) == ['batch_size', 'frame_id', 'metadata', 'points']
    annos = [{'score': np.zeros(3)}, {'score': np.zeros(2)}]
    text, d = ds.evaluation(annos, cfg.CLASS_NAMES)
    assert text == 'synthetic data: 5 detections over 2 frames (no ground truth, no mAP)\n' and d == {'num_detections': 5}
    cfg.DATA_CONFIG.SYNTHETIC.EVAL_GT = False
    ds0, _, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=False)
    assert sorted(ds0[1].keys()) == ['frame_id', 'metadata', 'points'] and np.array_equal(ds0[1]['points'], ds[1]['points'])
    cfg.DATA_CONFIG.SYNTHETIC.EVAL_GT = True
    ds1, loader1, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=False)
    train, _, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=True)
    assert np.array_equal(ds1[1]['gt_boxes'], train[1]['gt_boxes']) and np.array_equal(ds1[1]['points'], ds[1]['points'])
    assert next(iter(loader1))['gt_boxes'].shape[2] == 8
    # with the keyword the report is the evaluator's
    res = R.evaluate(R.make_case(8, [20], [10], list(cfg.CLASS_NAMES)), list(cfg.CLASS_NAMES))
    text, d = ds.evaluation(annos, cfg.CLASS_NAMES, device_eval=(res, 'report\n'))
    assert text.startswith('report\n') and 'mean_ap %.6f' % res['mean_ap'] in text and d['mAP'] == res['mean_ap'] and d['num_detections'] == 5
