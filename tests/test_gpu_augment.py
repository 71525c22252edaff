"""Device world augmentation on the GPU (csrc/augment.hip through pcp_amd/augment.py) against tests/golden/g26_augment.npz, the
reference's own DataAugmentor + mask_points_by_range on the same float32 inputs with the same drawn parameters: keep set and per-frame
counts exact, untouched columns bit-equal, coordinates / velocities / sizes within 4 ulp of the largest coordinate (|coords| <= 64),
angles within 1e-5, instances_tf within 16 * 2^-24 * max(1, largest |entry|) of the reference's float64 result.  Then one training
iteration of pointpillar_jr_corr_withmap and v2x_pointpillar_disco with the augmentor in the model function, and tools/train.py with
the switch set on the command line.  Every test prints its measured maxima before it asserts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_refs as ar
from helpers import load_golden
from pcp_amd import lib, synth
from pcp_amd.augment import DeviceWorldAugmentor

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
TILE_ROWS = lib.AUG_TILE_ROWS                      # rows one workgroup stages: the fixture's row counts are TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 1100
MASK = [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}]

D, META = ar.load_fixture()
CASES = list(META['cases'])


def _aug(name, **kw):
    m = META['cases'][name]
    return DeviceWorldAugmentor(m['cfg'], META['pc_range'], layout='nusc_map' if m['hd_map'] else 'car', data_processor=MASK, **kw)


def _setup(name):
    m = META['cases'][name]
    c = ar.case_arrays(D, name)
    aug = _aug(name)
    table = torch.from_numpy(aug.table(ar.params_of(c))).to(DEV)
    return m, c, aug, table


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('name', CASES)
def test_points_match_the_reference(name):
    assert TILE_ROWS == ar.TILE_ROWS
    m, c, aug, table = _setup(name)
    B = len(m['sizes'])
    pts = torch.from_numpy(c['points']).to(DEV)
    out, kept = aug.augment_points(pts, table, B)
    out2, kept2 = aug.augment_points(pts, table, B)
    full, none = aug.augment_points(pts, table, B, filter=False)
    torch.cuda.synchronize()
    assert torch.equal(pts.cpu(), torch.from_numpy(c['points']))              # the input is not written
    assert none is None and kept.tolist() == m['kept'] == kept2.tolist()
    got, got_full = out.cpu().numpy(), full.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(out2.cpu().numpy()))               # two runs, the same bits
    want_full = c['points_out']
    want = want_full[c['mask']]
    assert got.shape == want.shape and got_full.shape == want_full.shape
    assert np.array_equal(_bits(got), _bits(got_full[c['mask']]))              # the kept rows are the unfiltered call's rows, in order
    S = got_full.shape[1]
    angle_cols = ([10] if m['hd_map'] else []) + ([9] if S >= 14 else [])
    same = [k for k in range(S) if k not in (1, 2, 3) and k not in angle_cols]
    assert np.array_equal(_bits(got_full[:, same]), _bits(want_full[:, same]))    # frame, intensity, time, map masks, sweep, instance, agent
    e_xyz = float(np.abs(got_full[:, 1:4].astype(np.float64) - want_full[:, 1:4]).max(initial=0.0))
    e_ang = max([float(np.abs(got_full[:, k].astype(np.float64) - want_full[:, k]).max(initial=0.0)) for k in angle_cols] or [0.0])
    print('%s: %d rows, kept %s, max |xyz - reference| %.3g (bound %.3g), max |angle - reference| %.3g (bound %.3g)'
          % (name, got_full.shape[0], kept.tolist(), e_xyz, ar.COORD_TOL, e_ang, ar.ANGLE_TOL))
    assert e_xyz <= ar.COORD_TOL and e_ang <= ar.ANGLE_TOL
    if S >= 14:                                                                 # MoDAR heading: rows whose column -3 is 0 keep their bits
        plain = c['points'][:, S - 3] <= 0
        assert plain.any() and np.array_equal(_bits(got_full[plain, 9]), _bits(c['points'][plain, 9]))


@pytest.mark.parametrize('name', [n for n in CASES if n != 'empty'])
def test_boxes_and_instances_match_the_reference(name):
    m, c, aug, table = _setup(name)
    gt_in = torch.from_numpy(c['gt_boxes']).to(DEV)
    tf_in = torch.from_numpy(c['instances_tf']).to(DEV) if 'instances_tf' in c else None
    gt, tf = aug.augment_boxes(gt_in, tf_in, table)
    gt2, tf2 = aug.augment_boxes(gt_in, tf_in, table)
    torch.cuda.synchronize()
    assert torch.equal(gt, gt2) and (tf is None or torch.equal(tf, tf2))
    gt, want = gt.cpu().numpy(), c['gt_boxes_out']
    W = gt.shape[2]
    pad = c['gt_boxes'][..., W - 1] == 0
    assert pad.any() and np.array_equal(_bits(gt[pad]), _bits(c['gt_boxes'][pad])) and not gt[pad].any()
    assert np.array_equal(_bits(gt[..., W - 1]), _bits(c['gt_boxes'][..., W - 1]))
    lin = [0, 1, 2, 3, 4, 5] + ([7, 8] if W == 10 else [])
    e_box = float(np.abs(gt[..., lin].astype(np.float64) - want[..., lin]).max())
    e_head = float(np.abs(gt[..., 6].astype(np.float64) - want[..., 6]).max())
    e_tf, bound_tf = 0.0, ar.tf_tol(META['largest_tf'])
    if tf is not None:
        tf = tf.cpu().numpy()
        assert np.array_equal(_bits(tf[pad]), _bits(c['instances_tf'][pad]))
        if tf.shape[3] == 4:
            assert np.array_equal(_bits(tf[..., 3, :]), _bits(c['instances_tf'][..., 3, :]))
        e_tf = float(np.abs(tf.astype(np.float64) - c['instances_tf_out']).max())
        assert float(np.abs(c['instances_tf_out'] - c['instances_tf']).max()) > 0.1
    print('%s: boxes (B, M, %d): max |x y z dx dy dz vx vy - reference| %.3g (bound %.3g), heading %.3g (bound %.3g), instances_tf %.3g (bound %.3g)'
          % (name, W, e_box, ar.COORD_TOL, e_head, ar.ANGLE_TOL, e_tf, bound_tf))
    assert e_box <= ar.COORD_TOL and e_head <= ar.ANGLE_TOL and e_tf <= bound_tf


@pytest.mark.parametrize('name', ['w12', 'w13'])
def test_every_stage_disabled_returns_the_input_bits(name):
    m, c, aug, table = _setup(name)
    pts = torch.from_numpy(c['points']).to(DEV)
    out, kept = aug.augment_points(pts, table, len(m['sizes']), stages=[], filter=False)
    gt, tf = aug.augment_boxes(torch.from_numpy(c['gt_boxes']).to(DEV), torch.from_numpy(c['instances_tf']).to(DEV), table, stages=[])
    assert kept is None and np.array_equal(_bits(out.cpu().numpy()), _bits(c['points']))
    assert np.array_equal(_bits(gt.cpu().numpy()), _bits(c['gt_boxes'])) and np.array_equal(_bits(tf.cpu().numpy()), _bits(c['instances_tf']))


def test_compaction_over_many_tiles_is_the_unfiltered_result_masked():
    """140 001 rows of 7 floats: more than 256 tiles, so the place kernel's sum over the tiles in front of it takes more than one step per
    thread; the kept rows must be, bit for bit and in order, the rows of the unfiltered call that lie inside the range"""
    m, c, aug, table = _setup('w6')
    n = 140001
    rng = np.random.default_rng(5)
    pts = np.zeros((n, 7), dtype=np.float32)
    pts[:, 0] = np.sort(rng.integers(0, 3, n))
    pts[:, 1:3] = rng.uniform(-60, 60, (n, 2))
    pts[:, 3] = rng.uniform(-7, 5, n)
    pts[:, 4:] = rng.uniform(0, 1, (n, 3))
    dev = torch.from_numpy(pts).to(DEV)
    out, kept = aug.augment_points(dev, table, 3)
    full, _ = aug.augment_points(dev, table, 3, filter=False)
    full = full.cpu().numpy()
    r = np.asarray(META['pc_range'], dtype=np.float32)
    keep = np.ones(n, dtype=bool)
    for a in range(3):
        keep &= (full[:, 1 + a] >= r[a]) & (full[:, 1 + a] < r[a + 3])
    assert n // TILE_ROWS > 256 and 0.2 * n < keep.sum() < 0.9 * n
    assert kept.tolist() == [int(keep[pts[:, 0] == b].sum()) for b in range(3)]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(full[keep]))
    want, _ = ar.restate_points(pts, aug.table(ar.params_of(c)), aug.stages, False)
    assert float(np.abs(full[:, 1:4] - want[:, 1:4]).max()) <= ar.COORD_TOL


def test_refusals_on_the_host():
    m, c, aug, table = _setup('w7')
    with pytest.raises(ValueError, match='4 .*15'):
        aug.augment_points(torch.zeros(10, 3, device=DEV), table, 3)
    with pytest.raises(ValueError, match=r'\(8, 10\)'):
        aug.augment_boxes(torch.zeros(3, 4, 9, device=DEV), None, table)
    with pytest.raises(ValueError, match=r'\(3, 4\)'):
        aug.augment_boxes(torch.zeros(3, 4, 8, device=DEV), torch.zeros(3, 4, 2, 5, 4, device=DEV), table)
    with pytest.raises(ValueError, match='instances_tf'):
        aug.augment_boxes(torch.zeros(3, 4, 8, device=DEV), torch.zeros(3, 4, 2, 4, device=DEV), table)


def test_apply_updates_the_batch_like_the_reference():
    """apply() on a collated batch: points, gt_boxes, instances_tf and the per-frame parameters; se3_from_ego to 1e-12"""
    m, c, aug, _table = _setup('w13')
    p = ar.params_of(c)
    keys = [int(k) for k in c['se3_keys']]
    B = len(m['sizes'])
    bd = {'batch_size': B, 'points': torch.from_numpy(c['points']).to(DEV), 'gt_boxes': torch.from_numpy(c['gt_boxes']).to(DEV),
          'instances_tf': torch.from_numpy(c['instances_tf']).to(DEV),
          'metadata': [{'se3_from_ego': {k: c['se3'][b, i].copy() for i, k in enumerate(keys)}, 'lidar_id': 1} for b in range(B)]}
    aug.apply(bd, p)
    assert bd['points'].shape[0] == int(c['mask'].sum()) and bd['aug_points_kept'].tolist() == m['kept']
    assert float(np.abs(bd['points'].cpu().numpy()[:, 1:4] - c['points_out'][c['mask']][:, 1:4]).max()) <= ar.COORD_TOL
    assert float(np.abs(bd['gt_boxes'].cpu().numpy()[..., :6] - c['gt_boxes_out'][..., :6]).max()) <= ar.COORD_TOL
    assert float(np.abs(bd['instances_tf'].cpu().numpy() - c['instances_tf_out']).max()) <= ar.tf_tol(META['largest_tf'])
    for b in range(B):
        assert bd['metadata'][b]['lidar_id'] == 1
        for i, k in enumerate(keys):
            assert float(np.abs(bd['metadata'][b]['se3_from_ego'][k] - c['se3_out'][b, i]).max()) <= 1e-12
    assert np.array_equal(bd['flip_x'], p['flip_x']) and np.array_equal(bd['flip_y'], p['flip_y'])
    assert np.array_equal(bd['noise_rot'], c['noise_rot']) and np.array_equal(bd['noise_scale'], c['noise_scale'])


# ---- model level ---------------------------------------------------------------------------------------------------------------------

NUSC_AUG = {'DISABLE_AUG_LIST': ['placeholder'],
            'AUG_CONFIG_LIST': [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']},
                                {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.7854, 0.7854]},
                                {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.9, 1.1]},
                                {'NAME': 'random_world_translation', 'NOISE_TRANSLATE_STD': [0.5, 0.5, 0.5]}]}
MINI_RANGE = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]


def _build(meta):
    from pcdet.models import build_network_from_meta
    model = build_network_from_meta(meta)
    st = synth.fill_state_dict(meta['state_shapes'], scheme=meta.get('weight_scheme', 'survey'))
    for k, v in meta.get('state_overrides', {}).items():
        st[k] = np.asarray(v, dtype=np.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.to(DEV)


def _one_iteration(meta, batch, aug_cfg, layout, seed):
    """one fp32 training iteration through model_fn_decorator(augmentor): (loss, augmented points, model)"""
    from pcdet.models import model_fn_decorator
    model = _build(meta)
    model.train()
    aug = DeviceWorldAugmentor(aug_cfg, meta['pc_range'], layout=layout, data_processor=MASK, seed=seed)
    bd = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    ret = model_fn_decorator(aug)(model, bd)
    ret.loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    return float(ret.loss.detach()), bd, model


def _model_level(meta, batch, aug_cfg, layout, eval_batch):
    la, bda, model = _one_iteration(meta, batch, aug_cfg, layout, 666)
    lb, bdb, _ = _one_iteration(meta, batch, aug_cfg, layout, 666)
    lc, bdc, _ = _one_iteration(meta, batch, aug_cfg, layout, 667)
    print('losses: seed 666 %r, seed 666 again %r, seed 667 %r; rows %d -> %d' % (la, lb, lc, batch['points'].shape[0], bda['points'].shape[0]))
    assert np.isfinite(la) and np.isfinite(lc)
    assert 0 < bda['points'].shape[0] < batch['points'].shape[0]                # the range filter dropped rows, not all of them
    assert torch.equal(bda['points'], bdb['points']) and torch.equal(bda['gt_boxes'], bdb['gt_boxes'])
    assert la == lb                                                               # the same seed: the same loss bits
    assert lc != la and not np.array_equal(bda['noise_rot'], bdc['noise_rot'])   # another seed: another batch, another loss
    model.eval()
    with torch.no_grad():
        preds, _ = model(eval_batch)
    torch.cuda.synchronize()
    assert len(preds) == eval_batch['batch_size']


def test_corrector_model_trains_one_augmented_iteration():
    """pointpillar_jr_corr_withmap at the small range of the existing training tests (SYNTHETIC.XY_HALF 6.5, range +-6 m), HD-map rows
    (lane_dir follows the flips and the rotation), 10-column boxes and instances_tf through the augmentor"""
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    g = load_golden('g24_corr_mini.npz')
    meta = dict(g['meta']['cases']['corr'])
    assert [float(v) for v in meta['pc_range']] == MINI_RANGE
    cfg = cfg_from_yaml_file(os.path.join(PKG, 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_corr_withmap.yaml'), EasyDict())
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_FRAME=600, NUM_FRAMES=2, DISTRIBUTION='uniform', XY_HALF=6.5)
    ds, _loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=True)
    batch = ds.collate_batch([ds[i] for i in range(2)])
    assert ds.layout == 'nusc_map' and batch['points'].shape[1] == 13 and batch['gt_boxes'].shape[2] == 10 and 'instances_tf' in batch
    eval_batch = {'points': torch.from_numpy(g['points'].copy()).to(DEV), 'batch_size': 2, 'metadata': [{}, {}]}
    _model_level(meta, batch, NUSC_AUG, ds.layout, eval_batch)


def test_disco_model_trains_one_augmented_iteration():
    """v2x_pointpillar_disco at mini size (g7_train: 25.6 m x 25.6 m, three agents) with the V2X-Sim list (flip, rotation +-pi/4, scaling):
    the agents' poses move with the cloud.  The mini range keeps most of the cloud under these ranges, so none is shrunk."""
    from pcdet.config import EasyDict, cfg_from_yaml_file
    g = load_golden('g7_train.npz')
    meta = g['meta']
    dc = cfg_from_yaml_file(os.path.join(PKG, 'tools', 'cfgs', 'dataset_configs', '_v2x_sim_common.yaml'), EasyDict())
    md = [{'se3_from_ego': {0: g['pose_0'], 2: g['pose_2']}}, {'se3_from_ego': {0: g['pose_0']}}]
    batch = {'points': g['points'], 'gt_boxes': g['gt_boxes'], 'batch_size': 2, 'metadata': md}
    eval_batch = {'points': torch.from_numpy(g['points'].copy()).to(DEV), 'batch_size': 2, 'metadata': md}
    _model_level(meta, batch, dc.DATA_AUGMENTOR, 'disco', eval_batch)


def test_train_py_with_the_switch_set_on_the_command_line(tmp_path):
    """two iterations of tools/train.py on the DiscoNet YAML with DEVICE_AUG set through --set.  This config lists no
    mask_points_and_boxes_outside_range (the reference's does not either), so the points launch runs with the filter off"""
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'train.py', '--cfg_file', 'cfgs/v2x_sim_models/v2x_pointpillar_disco.yaml', '--batch_size', '2', '--epochs', '1',
           '--fix_random_seed', '--output_dir', str(tmp_path), '--set', 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '4000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '4', 'DATA_CONFIG.SYNTHETIC.DEVICE_AUG', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "device world augmentation: stages ['random_world_flip', 'random_world_rotation', 'random_world_scaling'], range filter off" in log
    losses = [float(v) for v in re.findall(r'loss ([0-9.]+)  lr', log)]
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses), (losses, log[-1500:])
    ck = torch.load(os.path.join(str(tmp_path), 'ckpt', 'checkpoint_epoch_1.pth'), map_location='cpu', weights_only=False)
    assert ck['it'] == 2 and all(torch.isfinite(v).all() for v in ck['model_state'].values() if v.dtype.is_floating_point)
