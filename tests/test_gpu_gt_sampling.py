"""Device gt_sampling on the GPU (csrc/gt_sample.hip through pcp_amd/gt_sampler.py) against tests/golden/g27_gt_sampling.npz, the
reference's own DataBaseSampler on the same inputs with the same drawn candidates: accepted database indices exact, point rows, gt_boxes
(mapped velocity included) and instances_tf bit-equal, paddings as the collation writes them, a second call the same bits.  Then the
whole augmentor (paste, world stages, range mask) against DataAugmentor.forward + mask_points_by_range within the bounds of
tests/test_gpu_augment.py, the database builder against a numpy restatement, and tools/train.py with the switches set."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_refs as ar
import gt_sampling_refs as gr
from pcp_amd import lib
from pcp_amd.augment import DeviceWorldAugmentor
from pcp_amd.gt_sampler import DeviceGtDatabase

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
MINI_RANGE = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]
MASK = [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}]

D, META = gr.load_fixture()
CASES = list(META['cases'])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _batch(c, info, with_tf=True):
    B = len(info['n_own'])
    b = {'points': torch.from_numpy(c['points']).to(DEV), 'gt_boxes': torch.from_numpy(c['gt_boxes']).to(DEV), 'batch_size': B,
         'metadata': [{'tf_target_from_glob': c['tf_target_from_glob'][i]} for i in range(B)]}
    if with_tf:
        b['instances_tf'] = torch.from_numpy(c['instances_tf']).to(DEV)
    return b


@pytest.mark.parametrize('name', CASES)
def test_paste_matches_the_reference_bit_for_bit(name):
    info = META['cases'][name]
    c = gr.case_arrays(D, name)
    s = gr.sampler_of(c, info, DEV)
    rng = np.random.RandomState(info['seed'])
    classes = s.frame_gt_classes(torch.from_numpy(c['gt_boxes']))
    drawn = [s.draw(cls, rng) for cls in classes]
    out = s.apply(_batch(c, info), drawn)
    again = s.apply(_batch(c, info), drawn)
    torch.cuda.synchronize()
    B = len(info['n_own'])
    assert [t.cpu().tolist() for t in out['gt_sampled_db_index']] == info['accepted']
    assert [m['num_added_instances'] for m in out['metadata']] == c['added'].tolist() and out['gt_sampled_rows'].tolist() == info['added_rows']
    pts, gt, tf = out['points'].cpu().numpy(), out['gt_boxes'].cpu().numpy(), out['instances_tf'].cpu().numpy()
    print('%s: %d -> %d rows, accepted %s' % (name, c['points'].shape[0], pts.shape[0], c['added'].tolist()))
    assert pts.shape == c['points_out'].shape and np.array_equal(_bits(pts), _bits(c['points_out']))
    assert gt.shape == c['gt_boxes_out'].shape and np.array_equal(_bits(gt), _bits(c['gt_boxes_out']))
    assert tf.shape == c['instances_tf_out'].shape and np.array_equal(_bits(tf), _bits(c['instances_tf_out']))
    # own rows first and untouched, the pasted rows carry the frame index and num_original_instances + idx
    col = s.inst_col
    for b in range(B):
        rows = pts[pts[:, 0] == b]
        own = c['points'][c['points'][:, 0] == b]
        assert np.array_equal(_bits(rows[:own.shape[0]]), _bits(own))
        ids = rows[own.shape[0]:, col]
        assert ids.size == info['added_rows'][b] and (ids.size == 0 or (ids.min() == info['n_own'][b] and ids.max() == info['n_own'][b] + c['added'][b] - 1))
        n = info['n_own'][b] + int(c['added'][b])
        assert not gt[b, n:].any() and np.array_equal(tf[b, n:, :, :3, :3], np.broadcast_to(np.eye(3, dtype=np.float32), tf[b, n:, :, :3, :3].shape))
        assert not tf[b, n:, :, :, 3].any() and (tf.shape[3] == 3 or not tf[b, n:, :, 3, :].any())
    assert np.array_equal(_bits(pts), _bits(again['points'].cpu().numpy())) and torch.equal(out['gt_boxes'], again['gt_boxes'])
    assert torch.equal(out['instances_tf'], again['instances_tf'])
    # instances_tf may be absent
    no_tf = s.apply(_batch(c, info, with_tf=False), drawn)
    assert 'instances_tf' not in no_tf and torch.equal(no_tf['gt_boxes'], out['gt_boxes']) and torch.equal(no_tf['points'], out['points'])
    # the inputs are not written
    fresh = _batch(c, info)
    s.apply(dict(fresh), drawn)
    assert torch.equal(fresh['points'].cpu(), torch.from_numpy(c['points'])) and torch.equal(fresh['gt_boxes'].cpu(), torch.from_numpy(c['gt_boxes']))


def test_descending_frame_rows_raise():
    info = META['cases']['s7']
    c = gr.case_arrays(D, 's7')
    s = gr.sampler_of(c, info, DEV)
    drawn = gr.drawn_of(s, info)
    b = _batch(c, info)
    b['points'] = torch.flip(b['points'], dims=[0]).contiguous()
    with pytest.raises(ValueError, match='ascending frame'):
        s.apply(b, drawn)
    b = _batch(c, info)
    b['points'][0, 0] = 7.0                                      # a frame index outside the batch
    with pytest.raises(ValueError, match='ascending frame'):
        s.apply(b, drawn)
    out = s.apply(_batch(c, info), drawn)                        # the error word is cleared by the next call
    assert np.array_equal(_bits(out['points'].cpu().numpy()), _bits(c['points_out']))


def test_limits_are_refused_with_their_numbers():
    info = META['cases']['s7']
    c = gr.case_arrays(D, 's7')
    s = gr.sampler_of(c, info, DEV)
    drawn = gr.drawn_of(s, info)
    b = _batch(c, info)
    many = [dict(d, groups=[np.arange(5).repeat(13), d['groups'][1], d['groups'][2]]) for d in drawn]
    with pytest.raises(ValueError, match='65 candidates.*%d' % lib.GTS_MAX_CAND):
        s.apply(b, many)
    with pytest.raises(ValueError, match=str(lib.GTS_MAX_BOXES)):
        s.apply(b, [dict(d, n_own=511) for d in drawn])
    wide = dict(b, points=torch.zeros((4, 16), device=DEV))
    with pytest.raises(ValueError, match=str(lib.AUG_MAX_ROW_STRIDE)):
        s.apply(wide, drawn)
    with pytest.raises(ValueError, match='database rows'):
        s.apply(dict(b, points=torch.zeros((4, 9), device=DEV)), drawn)
    with pytest.raises((lib.PcpError, RuntimeError)):
        s.apply(dict(b, points=b['points'].cpu()), drawn)
    with pytest.raises(ValueError, match='tf_target_from_glob'):
        i12, c12 = META['cases']['s12'], gr.case_arrays(D, 's12')
        s12 = gr.sampler_of(c12, i12, DEV)
        s12.apply(dict(_batch(c12, i12), metadata=[{}, {}, {}]), gr.drawn_of(s12, i12))


def test_whole_augmentor_matches_the_reference_forward():
    """paste, then flip / rotation / scaling, then the range mask, with RandomState(seed) drawing what the reference drew"""
    info = META['cases']['s12']
    c = gr.case_arrays(D, 's12')
    s = gr.sampler_of(c, info, DEV)
    aug = DeviceWorldAugmentor(info['aug_cfg'], META['pc_range'], layout='nusc_map', data_processor=MASK, gt_sampler=s)
    out = aug(_batch(c, info), rng=np.random.RandomState(info['aug_seed']))
    torch.cuda.synchronize()
    assert [t.cpu().tolist() for t in out['gt_sampled_db_index']] == info['aug_accepted']
    assert np.array_equal(out['flip_x'], c['aug_flip_x'].astype(bool)) and np.array_equal(out['noise_rot'], c['aug_noise_rot'])
    want_full, mask = c['aug_points_out'], c['aug_mask']
    want = want_full[mask]
    got = out['points'].cpu().numpy()
    assert out['aug_points_kept'].tolist() == info['aug_kept'] and got.shape == want.shape          # the keep sets are equal
    S = got.shape[1]
    same = [k for k in range(S) if k not in (1, 2, 3, 10)]
    assert np.array_equal(_bits(got[:, same]), _bits(want[:, same]))
    e_xyz = float(np.abs(got[:, 1:4].astype(np.float64) - want[:, 1:4]).max())
    e_ang = float(np.abs(got[:, 10].astype(np.float64) - want[:, 10]).max())
    gt, gt_want = out['gt_boxes'].cpu().numpy(), c['aug_gt_boxes_out']
    assert gt.shape == gt_want.shape and np.array_equal(_bits(gt[..., 9]), _bits(gt_want[..., 9]))
    lin = [0, 1, 2, 3, 4, 5, 7, 8]
    e_box = float(np.abs(gt[..., lin].astype(np.float64) - gt_want[..., lin]).max())
    e_head = float(np.abs(gt[..., 6].astype(np.float64) - gt_want[..., 6]).max())
    tf = out['instances_tf'].cpu().numpy()
    e_tf, bound_tf = float(np.abs(tf.astype(np.float64) - c['aug_instances_tf_out']).max()), ar.tf_tol(info['largest_tf'])
    print('s12 augmented: kept %s, xyz %.3g (bound %.3g), lane_dir %.3g, box %.3g, heading %.3g (bound %.3g), instances_tf %.3g (bound %.3g)'
          % (info['aug_kept'], e_xyz, ar.COORD_TOL, e_ang, e_box, e_head, ar.ANGLE_TOL, e_tf, bound_tf))
    assert e_xyz <= ar.COORD_TOL and e_ang <= ar.ANGLE_TOL and e_box <= ar.COORD_TOL and e_head <= ar.ANGLE_TOL and e_tf <= bound_tf


def _nusc_dataset(frames, boxes=40):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    cfg = cfg_from_yaml_file(os.path.join(PKG, 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_corr_withmap.yaml'), EasyDict())
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_FRAME=600, NUM_FRAMES=frames, DISTRIBUTION='uniform', XY_HALF=6.5, GT_BOXES=boxes)
    ds, _loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=True)
    return ds, cfg


def test_build_from_dataset_matches_a_numpy_restatement():
    from oracle.exchange import points_in_boxes
    ds, cfg = _nusc_dataset(2)
    db, infos = DeviceGtDatabase.build_from_dataset(ds, 2, min_points=1, device=DEV)
    assert ds.layout == 'nusc_map' and db.columns == 12 and db.boxes.shape[1] == 9 and db.n_sweeps == 10
    want = []
    for index in range(2):
        item = ds[index]
        gt, pts = item['gt_boxes'], item['points']
        assert item['metadata']['tf_target_from_glob'].shape == (4, 4) and item['metadata']['tf_target_from_glob'].dtype == np.float64
        assign = points_in_boxes(pts[:, :3], gt[:, :7])
        R = item['metadata']['tf_target_from_glob'][:3, :3]
        for j in range(gt.shape[0]):
            rows = np.nonzero(assign == j)[0]
            if rows.size == 0:
                continue
            obj = pts[rows].copy()
            obj[:, :3] = obj[:, :3] - gt[j, :3]
            want.append((cfg.CLASS_NAMES[int(gt[j, 9]) - 1], index, j, obj, np.linalg.inv(R) @ np.array([gt[j, 7], gt[j, 8], 0.0])))
    flat = [r for recs in infos.values() for r in recs]
    got_keys = sorted((r['name'], r['frame'], r['gt_idx']) for r in flat)
    assert got_keys == sorted((w[0], w[1], w[2]) for w in want) and len(db) == len(want) > 4          # the row sets: every object, once
    all_pts = db.points_dev.cpu().numpy()
    by_key = {(w[1], w[2]): w for w in want}
    k = 0
    for recs in infos.values():
        for r in recs:                                            # from_infos keeps this order
            w = by_key[(r['frame'], r['gt_idx'])]
            lo = int(db.offsets[k])
            assert db.counts[k] == w[3].shape[0] == r['num_points_in_gt'] and db.names[k] == w[0]
            assert np.array_equal(_bits(all_pts[lo:lo + int(db.counts[k])]), _bits(w[3]))             # centred coordinates bit-equal
            assert np.abs(db.velo[k] - w[4]).max() <= 1e-12 and r['instance_tf'].shape == (10, 4, 4)
            k += 1
    assert int(db.counts.sum()) == all_pts.shape[0]
    # eval items keep their bytes: no pose key outside training
    from pcdet.datasets import build_dataloader
    ev, _l, _s = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=False)
    assert 'tf_target_from_glob' not in ev[0]['metadata']


def _train(tmp_path, tag):
    tools = os.path.join(PKG, 'tools')
    out = os.path.join(str(tmp_path), tag)
    cmd = [sys.executable, 'train.py', '--cfg_file', 'cfgs/nuscenes_models/pointpillar_jr_corr_withmap.yaml', '--batch_size', '2', '--epochs', '1',
           '--fix_random_seed', '--output_dir', out, '--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE),
           'DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME', '600', 'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '4', 'DATA_CONFIG.SYNTHETIC.XY_HALF', '6.5',
           'DATA_CONFIG.SYNTHETIC.DISTRIBUTION', 'uniform', 'DATA_CONFIG.SYNTHETIC.GT_BOXES', '5', 'DATA_CONFIG.SYNTHETIC.GT_DROP_UNSTOCKED_GROUPS', 'True', 'DATA_CONFIG.SYNTHETIC.DEVICE_AUG', 'True', 'DATA_CONFIG.SYNTHETIC.DEVICE_GT_SAMPLING', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    return log, out


def test_train_py_with_gt_sampling_set_on_the_command_line(tmp_path):
    """one fp32 iteration of pointpillar_jr_corr_withmap at the mini range, twice with the same seed; the model-level half below checks the
    number of pasted instances and eval() afterwards"""
    log, out = _train(tmp_path, 'a')
    log2, _ = _train(tmp_path, 'b')
    assert 'device gt_sampling: database sizes' in log and "'gt_sampling', 'random_world_flip'" in log
    pasted = re.findall(r'first batch pasted (\d+) instances, (\d+) rows', log)
    assert len(pasted) == 1 and int(pasted[0][0]) > 0 and int(pasted[0][1]) > 0 and pasted == re.findall(r'first batch pasted (\d+) instances, (\d+) rows', log2)
    losses = re.findall(r'loss ([0-9.]+)  lr', log)
    # the first iteration is the one the seed determines: the weights two seeded runs hold after an optimizer step were seen to differ in
    # their last bits (with and without the paste), so a later iteration's loss may differ in its last printed digit
    assert len(losses) >= 1 and all(np.isfinite(float(v)) for v in losses) and losses[0] == re.findall(r'loss ([0-9.]+)  lr', log2)[0]
    a = torch.load(os.path.join(out, 'ckpt', 'checkpoint_epoch_1.pth'), map_location='cpu', weights_only=False)
    assert all(torch.isfinite(v).all() for v in a['model_state'].values() if v.dtype.is_floating_point)


def test_model_trains_one_iteration_with_pasted_objects_then_evaluates():
    import logging
    from helpers import load_golden
    from pcdet.models import build_network_from_meta, model_fn_decorator
    from pcp_amd import synth
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    import train as train_py
    g = load_golden('g24_corr_mini.npz')
    meta = dict(g['meta']['cases']['corr'])
    assert [float(v) for v in meta['pc_range']] == MINI_RANGE
    ds, cfg = _nusc_dataset(4, boxes=5)             # 5, 4, 3, 2 boxes: the 12 m range has room for pasted ones
    cfg.DATA_CONFIG.SYNTHETIC.DEVICE_GT_SAMPLING, cfg.DATA_CONFIG.SYNTHETIC.GT_DATABASE_FRAMES = True, 8
    cfg.DATA_CONFIG.SYNTHETIC.GT_DROP_UNSTOCKED_GROUPS = True
    log = logging.getLogger('gt_sampling_test')
    losses, added = [], []
    for _ in range(2):
        sampler = train_py.build_gt_sampler(cfg, ds, log)
        aug = DeviceWorldAugmentor.from_dataset_cfg(cfg.DATA_CONFIG, layout=ds.layout, seed=666, gt_sampler=sampler)
        assert aug.gt_sampler is sampler and aug.filter
        model = build_network_from_meta(meta)
        st = synth.fill_state_dict(meta['state_shapes'], scheme=meta.get('weight_scheme', 'survey'))
        for k, v in meta.get('state_overrides', {}).items():
            st[k] = np.asarray(v, dtype=np.float32)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        model = model.to(DEV).train()
        batch = ds.collate_batch([ds[i] for i in range(2)])
        ret = model_fn_decorator(aug)(model, batch)
        ret.loss.backward()
        torch.cuda.synchronize()
        losses.append(float(ret.loss.detach()))
        added.append(sum(m['num_added_instances'] for m in batch['metadata']))
    print('loss %r, pasted instances %r' % (losses, added))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]                      # the same seed: the same loss bits
    assert added[0] == added[1] and added[0] > 0
    model.eval()
    with torch.no_grad():
        pred, _ = model({'points': torch.from_numpy(g['points'].copy()).to(DEV), 'batch_size': 2, 'metadata': [{}, {}]})
    torch.cuda.synchronize()
    assert len(pred) == 2
