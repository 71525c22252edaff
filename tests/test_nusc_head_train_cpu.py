"""The float64 numpy statements of tests/nusc_head_refs.py reproduce what the reference's own six-head CenterHead (vel + iou branches)
produced on fixture g21 (tests/golden/make_golden_nusc_train.py) -- they ARE the reference's arithmetic -- plus the host rules of the
multi-head training path: the in-place class rewrite rule and the width check."""
import json

import numpy as np
import pytest
import torch

import nusc_head_refs as refs
from helpers import load_golden


@pytest.fixture(scope='module')
def g21():
    g = load_golden('g21_nusc_head_train.npz')
    g.update(load_golden('g21_nusc_head_train_grads.npz'))
    return g


def geom_of(meta, hw):
    ta = meta['dense_head']['TARGET_ASSIGNER_CONFIG']
    return dict(h=hw, w=hw, stride=float(ta['FEATURE_MAP_STRIDE']), voxel_x=float(np.float32(meta['voxel_size'][0])),
                voxel_y=float(np.float32(meta['voxel_size'][1])), min_x=meta['pc_range'][0], min_y=meta['pc_range'][1],
                overlap=float(ta['GAUSSIAN_OVERLAP']), min_radius=int(ta['MIN_RADIUS']))


def channels_of(meta, hi):
    """branch -> first channel of head hi's NHWC maps, regression channels in HEAD_ORDER concatenation order, number of classes"""
    hd = meta['dense_head']['SEPARATE_HEAD_CFG']['HEAD_DICT']
    names = meta['branch_names'][hi]
    ncls = len(meta['dense_head']['CLASS_NAMES_EACH_HEAD'][hi])
    outs = [ncls if n == 'hm' else hd[n]['out_channels'] for n in names]
    offs = np.concatenate([[0], np.cumsum(outs)]).astype(int)
    off = {n: int(o) for n, o in zip(names, offs[:-1])}
    reg = []
    for n in meta['dense_head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']:
        reg += [off[n] + j for j in range(outs[names.index(n)])]
    return off, reg, ncls


def ref_targets(g):
    meta = g['meta']
    heads = []
    for hi in range(meta['n_heads']):
        off, _reg, _ncls = channels_of(meta, hi)
        heads.append(dict(maps=g['h%d_maps' % hi], center=off['center'], center_z=off['center_z'], dim=off['dim'], rot=off['rot']))
    tables = refs.class_tables(meta['class_names'], meta['dense_head']['CLASS_NAMES_EACH_HEAD'])
    K = int(meta['dense_head']['TARGET_ASSIGNER_CONFIG']['NUM_MAX_OBJS'])
    return refs.assign_targets(g['gt_boxes'], tables, geom_of(meta, g['h0_maps'].shape[1]), K, heads=heads)


def test_fixture_holds_the_planted_cases(g21):
    g = g21
    masks = [g['h%d_mask' % h] for h in range(6)]
    assert masks[3][0].sum() == 0 and masks[3][2].sum() > 0                          # a head with no box in one frame
    assert masks[0][1].sum() > 0 and all(masks[h][1].sum() == 0 for h in range(1, 6))  # a frame whose boxes all belong to one head
    gt = g['gt_boxes']
    cls0 = gt[0, :, 9]
    nz = np.nonzero(cls0)[0]
    assert (cls0[nz[0]:nz[-1]] == 0).any()                                           # padding rows between valid rows
    assert ((gt[..., 3] == 0) & (gt[..., 9] > 0)).any()                              # a dx = 0 box ...
    assert masks[0][0, :int((cls0 == 1).sum())].min() == 0                           # ... whose slot stays empty
    i1 = g['h1_inds'][0][masks[1][0] > 0]
    assert len(set(i1.tolist())) < len(i1)                                           # two boxes of one head in one cell
    assert (g['h1_heat'][0] == 1).any(axis=(0, 1)).all()                             # both classes of a two-class head
    assert (gt[..., 0] > 12.8).any() and (g['h4_inds'][0][masks[4][0] > 0] % 32 == 31).any()   # clamped centre
    assert (g['h5_inds'][0][masks[5][0] > 0] == 31 * 32).any()                       # on the map edge
    # the reference rewrote the class column in place, and for this head list that changed no assignment (checked below against gt_boxes)
    assert not np.array_equal(g['gt_class_after_reference'], gt[..., 9])
    assert float(g['iou_f32_gap']) < 1e-5


def test_numpy_targets_reproduce_the_reference(g21):
    g = g21
    want = ref_targets(g)
    gap = max(2e-6, 4 * float(g['iou_f32_gap']))
    for hi, w in enumerate(want):
        assert np.array_equal(w['inds'], g['h%d_inds' % hi]) and np.array_equal(w['mask'], g['h%d_mask' % hi]), hi
        heat = g['h%d_heat' % hi]
        assert np.array_equal(w['heat'] == 1.0, heat == 1.0), hi
        np.testing.assert_allclose(w['heat'], heat, rtol=0, atol=1e-6)
        assert w['tb'].shape == g['h%d_tb' % hi].shape == (3, 500, 11)
        np.testing.assert_allclose(w['tb'][..., :10], g['h%d_tb' % hi][..., :10], rtol=0, atol=2e-6)
        np.testing.assert_allclose(w['tb'][..., 10], g['h%d_tb' % hi][..., 10], rtol=0, atol=gap)
        m = w['mask'] > 0
        if m.any():
            assert np.abs(w['tb'][..., 10][m]).max() <= 1.0


def test_numpy_losses_and_gradients_reproduce_the_reference(g21):
    g = g21
    meta = g['meta']
    lw = meta['dense_head']['LOSS_CONFIG']['LOSS_WEIGHTS']
    tb_ref = json.loads(str(g['tb_json']))
    total = np.float32(0)
    for hi in range(meta['n_heads']):
        off, reg, ncls = channels_of(meta, hi)
        r = refs.head_loss(g['h%d_maps' % hi], off['hm'], ncls, reg, g['h%d_heat' % hi], g['h%d_tb' % hi].astype(np.float64),
                           g['h%d_inds' % hi], g['h%d_mask' % hi], lw['code_weights'], lw['cls_weight'], lw['loc_weight'])
        for key, v in (('hm_loss_head_%d' % hi, r['hm']), ('loc_loss_head_%d' % hi, r['loc'])):
            assert abs(v - tb_ref[key]) <= 2e-5 * max(abs(tb_ref[key]), 1e-3), (key, v, tb_ref[key])
        assert r['num_pos'] == int((g['h%d_heat' % hi] == 1).sum())
        ref = g['h%d_dmaps' % hi].astype(np.float64)
        assert np.abs(r['dmaps'] - ref).max() <= 2e-4 * max(np.abs(ref).max(), 1e-6), hi
        total = np.float32(total + np.float32(r['hm'] + r['loc']))
    assert abs(float(total) - tb_ref['rpn_loss']) <= 2e-5 * abs(tb_ref['rpn_loss'])
    assert abs(float(g['loss']) - tb_ref['rpn_loss']) <= 1e-6 * abs(tb_ref['rpn_loss'])


def test_numpy_targets_rank_cut_and_single_row():
    """K = 8 with more than 8 boxes of one head: ranks >= K are dropped (the boxes of the other head do not use up slots); M = 1"""
    names = ['car', 'truck', 'bus']
    tables = refs.class_tables(names, [['car'], ['truck', 'bus']])
    geom = dict(h=16, w=16, stride=4.0, voxel_x=0.2, voxel_y=0.2, min_x=-6.4, min_y=-6.4, overlap=0.1, min_radius=2)
    rs = np.random.RandomState(3)
    gt = np.zeros((1, 20, 8), dtype=np.float32)
    gt[0, :, :2] = rs.uniform(-6, 6, (20, 2))
    gt[0, :, 3:6] = rs.uniform(0.5, 3, (20, 3))
    gt[0, :, 7] = [1, 2, 1, 1, 3, 1, 1, 1, 2, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1]
    out = refs.assign_targets(gt, tables, geom, 8)
    assert out[0]['mask'].sum() == 8 and out[1]['mask'].sum() == 4 and out[0]['tb'].shape == (1, 8, 8)
    cars = np.nonzero(gt[0, :, 7] == 1)[0][:8]
    cx = np.clip((gt[0, cars, 0].astype(np.float64) + 6.4) / 0.2 / 4, 0, 15.5).astype(int)
    cy = np.clip((gt[0, cars, 1].astype(np.float64) + 6.4) / 0.2 / 4, 0, 15.5).astype(int)
    assert np.array_equal(out[0]['inds'][0], cy * 16 + cx)
    one = refs.assign_targets(gt[:, 4:5], tables, geom, 8)
    assert one[0]['mask'].sum() == 0 and one[1]['mask'].sum() == 1 and (one[1]['heat'][..., 1] == 1).sum() == 1


def test_class_rewrite_rule():
    from pcdet.models.dense_heads.center_head import check_class_rewrite_is_inert, class_rewrite_is_inert
    names = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
    shipped = [['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
               ['pedestrian', 'traffic_cone']]
    assert class_rewrite_is_inert(names, shipped)
    check_class_rewrite_is_inert(names, shipped)
    assert class_rewrite_is_inert(['car'], [['car']]) and class_rewrite_is_inert(['car', 'truck'], [['car', 'truck']])
    # a later head holds `car`: the rows the first head rewrote to 1 would be taken again as cars
    planted = [['truck', 'construction_vehicle'], ['car'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
               ['pedestrian', 'traffic_cone']]
    assert not class_rewrite_is_inert(names, planted)
    with pytest.raises(NotImplementedError, match='rewrites the class column'):
        check_class_rewrite_is_inert(names, planted)
    # ... and `truck` (v = 2) behind a two-class head
    assert not class_rewrite_is_inert(names, [['bus', 'trailer'], ['truck'], ['car']] + [[n] for n in names if n not in
                                                                                          ('bus', 'trailer', 'truck', 'car')])


def test_width_mismatch_is_a_value_error():
    from pcp_amd import lib
    from pcp_amd import train_ops as tops
    z = torch.zeros
    head = dict(head=z((1, 4, 4, 16)), heat=z((1, 4, 4, 1)), tb=z((1, 8, 10)), inds=z((1, 8), dtype=torch.int32),
                mask=z((1, 8), dtype=torch.int32), ch_hm=11, num_class=1, reg_ch=list(range(11)))
    with pytest.raises(ValueError, match='10 columns'):
        tops.centerhead_loss_ext(lib.HeadLossExt(), [head])
    with pytest.raises(ValueError):
        tops.centerhead_target_width(9, False)
    assert [tops.centerhead_target_width(w, i) for w in (8, 10) for i in (False, True)] == [8, 9, 10, 11]
    with pytest.raises(ValueError):
        refs.head_loss(np.zeros((1, 4, 4, 16)), 11, 1, list(range(11)), np.zeros((1, 4, 4, 1)), np.zeros((1, 8, 10)), None, None, [1] * 11, 1, 1)


def test_code_width_pairing_is_settled_before_anything_runs(g21):
    """vel in HEAD_ORDER with 8-column boxes (target_boxes would have 9 columns against 11 channels): a ValueError from the forward itself,
    on the host, before any launch -- CPU tensors never reach a kernel"""
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads.center_head import CenterHead
    meta = g21['meta']
    head = CenterHead(EasyDict(meta['dense_head']), 384, 10, meta['class_names'], np.array(meta['grid_size']),
                      np.array(meta['pc_range'], dtype=np.float32), meta['voxel_size'], predict_boxes_when_training=False).train()
    batch = {'spatial_features_2d': torch.zeros((1, 384, 32, 32)), 'gt_boxes': torch.zeros((1, 4, 8)), 'batch_size': 1}
    with pytest.raises(ValueError, match='target_boxes of 9 columns'):
        head(batch)
    head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['code_weights'] = [1.0] * 8
    with pytest.raises(ValueError, match='code_weights has 8 entries'):
        head(dict(batch, gt_boxes=torch.zeros((1, 4, 10))))


def test_model_fixture_is_composed_from_the_shipped_yaml_sections():
    """fixture (b): VFE, MAP_TO_BEV and BACKBONE_2D of v2x_sim_models/_pointpillar_trunk.yaml, DENSE_HEAD of
    nuscenes_models/_pointpillar_jr_trunk.yaml -- no new YAML"""
    import os
    import yaml
    cfgs = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'practical-collab-perception_amd', 'tools', 'cfgs')
    trunk = yaml.safe_load(open(os.path.join(cfgs, 'v2x_sim_models', '_pointpillar_trunk.yaml')))
    nusc = yaml.safe_load(open(os.path.join(cfgs, 'nuscenes_models', '_pointpillar_jr_trunk.yaml')))
    meta = load_golden('g21_nusc_model_train.npz')['meta']
    for key in ('VFE', 'MAP_TO_BEV', 'BACKBONE_2D'):
        assert meta['model'][key] == trunk[key], key
    assert meta['model']['DENSE_HEAD'] == nusc['DENSE_HEAD'] and len(meta['class_names']) == 10
    assert meta['pc_range'][3] - meta['pc_range'][0] == 12.8                      # 64 x 64 pillars of 0.2 m
