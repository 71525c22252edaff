"""Per-object device augmentation on the GPU (csrc/object_augment.hip through pcp_amd/object_augment.py and DeviceWorldAugmentor) against
tests/golden/g28_object_augment.npz, the reference's own functions on the same float32 inputs with the same drawn values: surviving
rows and boxes and their order exact, untouched columns and padding bit-equal, translations bit-equal, rotation / scaling coordinates
and the box columns within XYZ_BOUND / BOX_BOUND.  Every test prints its measured maxima before it asserts.

Measured on the MI355X against the fixture, maxima over all cases: point xyz 3.81e-06 (local scaling, and the full list), box columns
3.81e-06 (the world rotation of the full list; 0 in every object-only case); the bounds are ten times those, 3.81e-05 (floored at one
ulp of the largest coordinate, 64), so another correct operation order passes and a wrong centre or angle
(errors of 1e-2 and more) does not."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import object_augment_refs as oar
from pcp_amd import lib
from pcp_amd import object_augment as obj
from pcp_amd.augment import DeviceWorldAugmentor

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
MINI_RANGE = [-6.4, -6.4, -5.0, 6.4, 6.4, 3.0]             # the 12.8 m range of tests/golden/g24_corr_mini.npz
D, META = oar.load_fixture()
CASES = list(META['cases'])
ULP64 = 2.0 ** -23 * 64
MEASURED_XYZ, MEASURED_BOX = 3.81e-06, 3.81e-06
XYZ_BOUND, BOX_BOUND = max(10 * MEASURED_XYZ, ULP64), max(10 * MEASURED_BOX, ULP64)
EXACT = {'lt_x', 'lt_y', 'lt_z', 'ldrop_top', 'ldrop_bottom', 'ldrop_left', 'ldrop_right', 'wdrop_top', 'wdrop_bottom', 'wdrop_left', 'wdrop_right'}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _aug(name, **kw):
    return DeviceWorldAugmentor(META['cases'][name]['cfg'], META['pc_range'], object_stages=True, **kw)


def _batch(c):
    return {'points': torch.from_numpy(c['points']).to(DEV), 'gt_boxes': torch.from_numpy(c['gt_boxes']).to(DEV), 'batch_size': len(META['sizes'])}


def _compare(name, c, out, exact):
    pts, gt = out['points'].cpu().numpy(), out['gt_boxes'].cpu().numpy()
    want, want_gt = c['points_out'], c['gt_boxes_out']
    assert pts.shape == want.shape, (pts.shape, want.shape)
    src = c['points'][c['kept_rows']]
    assert np.array_equal(_bits(pts[:, 0]), _bits(src[:, 0])) and np.array_equal(_bits(pts[:, 4:]), _bits(src[:, 4:]))     # rows, order, untouched columns
    assert np.array_equal(gt[..., -1], want_gt[..., -1])                                                                 # box survivors and order
    W = gt.shape[2]
    pad = want_gt[..., -1] == 0
    assert np.array_equal(_bits(gt[pad]), _bits(want_gt[pad]))
    if W == 10:
        assert np.array_equal(_bits(gt[..., 7:9]), _bits(want_gt[..., 7:9]))
    e_xyz = float(np.abs(pts[:, 1:4] - want[:, 1:4]).max(initial=0.0))
    e_box = float(np.abs(gt[..., :7] - want_gt[..., :7]).max(initial=0.0))
    print('%s: max |xyz - reference| = %.3g (bound %.3g), max |box - reference| = %.3g (bound %.3g)' % (name, e_xyz, XYZ_BOUND, e_box, BOX_BOUND))
    if exact:
        assert np.array_equal(_bits(pts[:, 1:4]), _bits(want[:, 1:4])) and np.array_equal(_bits(gt), _bits(want_gt))
    assert e_xyz <= XYZ_BOUND and e_box <= BOX_BOUND, (e_xyz, e_box)
    return e_xyz, e_box


@pytest.mark.parametrize('name', CASES)
def test_case_matches_the_reference(name):
    c = oar.case_arrays(D, name)
    aug = _aug(name)
    out = aug.apply(_batch(c), oar.params_of(META, name, c))
    torch.cuda.synchronize()
    assert [int(v) for v in (out['gt_boxes'][..., -1] != 0).sum(1).cpu()] == META['cases'][name]['boxes_kept']
    _compare(name, c, out, name in EXACT)
    if name == 'lscale_skip':                                    # the early return: no scaling stage ran
        assert aug.steps[0]['stages'] == [lib.OBJ_ROTATE]


def test_two_identical_calls_are_bit_equal_and_the_input_is_not_written():
    c = oar.case_arrays(D, 'full')
    p = oar.params_of(META, 'full', c)
    b1, b2 = _batch(c), _batch(c)
    keep = b1['points']
    o1, o2 = _aug('full').apply(b1, p), _aug('full').apply(b2, p)
    torch.cuda.synchronize()
    assert torch.equal(o1['points'].view(torch.int32), o2['points'].view(torch.int32)) and torch.equal(o1['gt_boxes'].view(torch.int32), o2['gt_boxes'].view(torch.int32))
    assert torch.equal(keep.cpu(), torch.from_numpy(c['points']))


def test_full_list_from_a_seed_through_call():
    c = oar.case_arrays(D, 'full')
    aug = _aug('full', seed=META['cases']['full']['seed'])
    bd = _batch(c)
    bd['num_gt_boxes'] = META['n_boxes']
    out = aug(bd)
    torch.cuda.synchronize()
    assert np.array_equal(out['flip_x'], c['flip_x'].astype(bool)) and np.array_equal(out['flip_y'], c['flip_y'].astype(bool))
    _compare('full (seeded)', c, out, False)


def test_a_row_pushed_out_of_one_box_into_the_next_is_moved_again():
    """boxes A = [0, 4] and B = [4.25, 8.25] along x (each 0.1 wider by the margin); a row at x = 3.75 goes +0.5 with A, lands in B at 4.25 and
    goes +0.25 with B.  With the boxes in the other order B sees it at 3.75, outside, and only A moves it.  Every value is a dyadic number."""
    gt = torch.tensor([[[2.0, 0, 0, 4, 2, 2, 0, 1], [6.25, 0, 0, 4, 2, 2, 0, 1]]], device=DEV)
    pts = torch.tensor([[0, 3.75, 0.5, 0.25, 9.0], [0, 20.0, 0, 0, 7.0]], device=DEV)
    vals = [np.asarray([[0.5, 0.25]])]
    out, g, _ = obj.local_stages(pts, gt, [lib.OBJ_TRANSLATE_X], vals)
    assert out.cpu().tolist() == [[0, 4.5, 0.5, 0.25, 9.0], [0, 20.0, 0, 0, 7.0]] and g[0, :, 0].cpu().tolist() == [2.5, 6.5]
    out, g, _ = obj.local_stages(pts, gt.flip(1), [lib.OBJ_TRANSLATE_X], [np.asarray([[0.25, 0.5]])])
    assert out.cpu().tolist() == [[0, 4.25, 0.5, 0.25, 9.0], [0, 20.0, 0, 0, 7.0]] and g[0, :, 0].cpu().tolist() == [6.5, 2.5]


def test_empty_frames_pass_the_world_dropout_untouched():
    gt = torch.from_numpy(oar.case_arrays(D, 'wdrop_top')['gt_boxes']).to(DEV)
    tf = torch.arange(gt.shape[0] * gt.shape[1] * 2 * 12, dtype=torch.float32, device=DEV).reshape(gt.shape[0], gt.shape[1], 2, 3, 4)
    pts = torch.zeros((0, 5), device=DEV)
    for d in (lib.OBJ_WORLD_DROP_TOP, lib.OBJ_WORLD_DROP_BOTTOM, lib.OBJ_WORLD_DROP_LEFT, lib.OBJ_WORLD_DROP_RIGHT):
        out, g, t, kept, n = obj.world_dropout(pts, gt, tf, d, [0.1] * gt.shape[0])
        assert out.shape == (0, 5) and kept.tolist() == [0, 0, 0] and n.cpu().tolist() == META['n_boxes']
        assert torch.equal(g.view(torch.int32), gt.view(torch.int32)) and torch.equal(t, tf) and not torch.isnan(g).any()
    ext = obj.frame_extent(torch.from_numpy(oar.case_arrays(D, 'wdrop_top')['points']).to(DEV), 3, 3).cpu().numpy()
    assert ext[1, 0] == np.inf and ext[1, 1] == -np.inf and np.isfinite(ext[[0, 2]]).all()


def test_instances_tf_rows_move_with_their_boxes():
    c = oar.case_arrays(D, 'wdrop_left')
    gt = torch.from_numpy(c['gt_boxes']).to(DEV)
    B, M = gt.shape[:2]
    tf = torch.zeros((B, M, 2, 4, 4), device=DEV)
    tf[..., 0, 3] = torch.arange(M, device=DEV, dtype=torch.float32).view(1, M, 1) + 100
    inten = oar.params_of(META, 'wdrop_left', c)['object'][0]
    out, g, t, kept, n = obj.world_dropout(torch.from_numpy(c['points']).to(DEV), gt, tf, lib.OBJ_WORLD_DROP_LEFT, [float(v[0]) for v in inten])
    assert n.cpu().tolist() == META['cases']['wdrop_left']['boxes_kept'] and kept.tolist() == META['cases']['wdrop_left']['kept']
    want = c['gt_boxes_out']
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(want))
    for b in range(B):
        if META['sizes'][b] == 0:                                # no extent: boxes and matrices are copied as they are
            assert torch.equal(t[b], tf[b])
            continue
        src = [m for m in range(M) if any(np.array_equal(c['gt_boxes'][b, m], w) for w in want[b, :int(n[b])])]
        assert t[b, :len(src), 0, 0, 3].cpu().tolist() == [100.0 + m for m in src]
        assert torch.equal(t[b, len(src):, :, :3, :3], torch.eye(3, device=DEV).expand(M - len(src), 2, 3, 3)) and (t[b, len(src):, :, :, 3] == 0).all()


@pytest.mark.parametrize('S', [14, 15])
def test_the_widest_rows_go_through_the_dropout_walk(S):
    """the fixture's ldrop_left rows (a dropout: both tile buffers in LDS) widened to 14 and 15 columns, the widest the kernels take"""
    c = oar.case_arrays(D, 'ldrop_left')
    extra = np.random.default_rng(S).uniform(-9, 9, (c['points'].shape[0], S - c['points'].shape[1])).astype(np.float32)
    wide = np.concatenate([c['points'], extra], axis=1)
    values = oar.params_of(META, 'ldrop_left', c)['object'][0]
    out, g, kept = obj.local_stages(torch.from_numpy(wide).to(DEV), torch.from_numpy(c['gt_boxes']).to(DEV), [lib.OBJ_DROP_LEFT], values)
    assert kept.tolist() == META['cases']['ldrop_left']['kept']
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(wide[c['kept_rows']]))


def test_rows_of_a_foreign_frame_are_kept_and_counted():
    """a row whose frame index lies outside [0, batch) passes a dropout call untouched and no real row is cut off behind it"""
    gt = torch.tensor([[[0.0, 0, 0, 4, 2, 2, 0, 1]]], device=DEV)
    pts = torch.tensor([[0, 0.5, 0, 0.75, 1.0], [5, 0.5, 0, 0.75, 2.0], [0, 0.5, 0, -0.5, 3.0], [0, 30.0, 0, 0, 4.0]], device=DEV)
    out, _, kept = obj.local_stages(pts, gt, [lib.OBJ_DROP_TOP], [np.asarray([[0.25]])])       # threshold z >= 1 - 0.5 = 0.5
    assert kept.tolist() == [2] and out.cpu().tolist() == [[5, 0.5, 0, 0.75, 2.0], [0, 0.5, 0, -0.5, 3.0], [0, 30.0, 0, 0, 4.0]]


def test_box_counts_read_back_in_the_middle_of_the_list():
    """a world dropout in front of local stages, one frame (the reference's per-sample draw order): __call__ draws the dropout, runs it,
    reads the box count (9 -> 8 in frame 0 of wdrop_left) and draws the local stages for the boxes that are left.  Expected: the numpy
    restatement fed from the same seed in the reference's order.  Then three frames: __call__ against apply() with the same values."""
    c = oar.case_arrays(D, 'wdrop_left')
    m = META['cases']['wdrop_left']
    cfg = [m['cfg'][0], {'NAME': 'random_local_translation', 'LOCAL_TRANSLATION_RANGE': [0.2, 0.9], 'ALONG_AXIS_LIST': ['x']},
           {'NAME': 'random_local_scaling', 'LOCAL_SCALE_RANGE': [0.8, 1.2]}]
    n0, nb0 = META['sizes'][0], META['n_boxes'][0]
    aug = DeviceWorldAugmentor(cfg, META['pc_range'], object_stages=True, seed=m['seed'])
    assert aug.splits == [1]
    out = aug({'points': torch.from_numpy(c['points'][:n0]).to(DEV), 'gt_boxes': torch.from_numpy(c['gt_boxes'][:1]).to(DEV), 'batch_size': 1})
    rs = np.random.RandomState(m['seed'])
    lo, hi = m['cfg'][0]['INTENSITY_RANGE']
    steps = [(oar.WORLD_DROP_LEFT, rs.uniform(lo, hi))]
    left = oar.restate_frame(c['points'][:n0, 1:], c['gt_boxes'][0, :nb0], steps)[1].shape[0]
    assert left == m['boxes_kept'][0] < nb0
    steps += [(oar.TRANSLATE_X, np.asarray([rs.uniform(0.2, 0.9) for _ in range(left)])), (oar.SCALE, np.asarray([rs.uniform(0.8, 1.2) for _ in range(left)]))]
    p, g, ids = oar.restate_frame(c['points'][:n0, 1:], c['gt_boxes'][0, :nb0], steps)
    got, got_g = out['points'].cpu().numpy(), out['gt_boxes'].cpu().numpy()[0]
    assert got.shape[0] == len(ids) and np.array_equal(_bits(got[:, 4:]), _bits(c['points'][:n0][ids][:, 4:]))
    g[:, 6] = oar.limit_period(g[:, 6])
    e_xyz, e_box = float(np.abs(got[:, 1:4] - p[:, :3]).max()), float(np.abs(got_g[:left] - g).max())
    print('split list, one frame: max |xyz - restatement| = %.3g, max |box - restatement| = %.3g (bounds %.3g)' % (e_xyz, e_box, XYZ_BOUND))
    assert e_xyz <= XYZ_BOUND and e_box <= BOX_BOUND and not got_g[left:].any()
    # three frames: the same values through apply()
    aug = DeviceWorldAugmentor(cfg, META['pc_range'], object_stages=True)
    rs = np.random.RandomState(m['seed'])                         # the fixture's intensities, hence its box counts after the dropout
    p1 = aug.draw(3, rs, n_boxes=META['n_boxes'], entries=(0, 1))
    params = aug.draw(3, rs, None, m['boxes_kept'], (1, 3), p1)
    a = aug.apply(_batch(c), params)
    b = aug(_batch(c), rng=np.random.RandomState(m['seed']))
    assert torch.equal(a['points'].view(torch.int32), b['points'].view(torch.int32)) and torch.equal(a['gt_boxes'].view(torch.int32), b['gt_boxes'].view(torch.int32))
    assert 'num_gt_boxes' not in b


def test_train_py_with_object_stages_set_on_the_command_line(tmp_path):
    """one epoch (two iterations) of tools/train.py on pointpillar_jr_corr_withmap at the mini range with a DATA_AUGMENTOR list that holds
    per-object stages (the shipped YAMLs list none, so the test writes a model YAML beside them that differs in that list only), DEVICE_AUG
    and DEVICE_OBJECT_AUG set through --set.  10-column boxes: every object stage but the local rotation."""
    import yaml
    tools = os.path.join(PKG, 'tools')
    with open(os.path.join(tools, 'cfgs', 'nuscenes_models', 'pointpillar_jr_corr_withmap.yaml')) as f:
        model_cfg = yaml.safe_load(f)
    model_cfg['DATA_CONFIG']['DATA_AUGMENTOR'] = {'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': [
        {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']},
        {'NAME': 'random_local_translation', 'LOCAL_TRANSLATION_RANGE': [-0.2, 0.2], 'ALONG_AXIS_LIST': ['x', 'y', 'z']},
        {'NAME': 'random_local_scaling', 'LOCAL_SCALE_RANGE': [0.9, 1.1]},
        {'NAME': 'random_local_frustum_dropout', 'INTENSITY_RANGE': [0.0, 0.2], 'DIRECTION': ['top']},
        {'NAME': 'random_world_frustum_dropout', 'INTENSITY_RANGE': [0.0, 0.1], 'DIRECTION': ['left']},
        {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.3925, 0.3925]}]}
    cfg_file = os.path.join(str(tmp_path), 'pointpillar_jr_corr_withmap_objaug.yaml')
    with open(cfg_file, 'w') as f:
        yaml.safe_dump(model_cfg, f)
    cmd = [sys.executable, 'train.py', '--cfg_file', cfg_file, '--batch_size', '2', '--epochs', '1', '--fix_random_seed', '--output_dir',
           os.path.join(str(tmp_path), 'out'), '--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE),
           'DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME', '600', 'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '4', 'DATA_CONFIG.SYNTHETIC.XY_HALF', '6.5',
           'DATA_CONFIG.SYNTHETIC.DISTRIBUTION', 'uniform', 'DATA_CONFIG.SYNTHETIC.GT_BOXES', '5', 'DATA_CONFIG.SYNTHETIC.DEVICE_AUG', 'True',
           'DATA_CONFIG.SYNTHETIC.DEVICE_OBJECT_AUG', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "'random_local_translation', 'random_local_scaling', 'random_local_frustum_dropout', 'random_world_frustum_dropout'" in log
    assert 'is not a world transform of the device path, skipped' not in log
    losses = [float(v) for v in re.findall(r'loss ([0-9.]+)  lr', log)]
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses), (losses, log[-1500:])
    ck = torch.load(os.path.join(str(tmp_path), 'out', 'ckpt', 'checkpoint_epoch_1.pth'), map_location='cpu', weights_only=False)
    assert all(torch.isfinite(v).all() for v in ck['model_state'].values() if v.dtype.is_floating_point)
