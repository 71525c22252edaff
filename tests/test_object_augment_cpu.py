"""Host side of the per-object device augmentation (pcp_amd/object_augment.py, DeviceWorldAugmentor(object_stages=True)) without a GPU:
the opt-in and the queue, draw() against the uniforms the reference drew from the same seed (tests/golden/g28_object_augment.npz), the
refusals, the symbols, and the numpy restatement tests/object_augment_refs.py against the fixture's outputs."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import object_augment_refs as oar
from pcp_amd import lib
from pcp_amd import object_augment as obj
from pcp_amd.augment import DeviceWorldAugmentor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, META = oar.load_fixture()
CASES = list(META['cases'])
OBJECT_ONLY = [n for n in CASES if all(c['NAME'] in oar.OBJECT_NAMES for c in META['cases'][n]['cfg'])]   # 'full' also has world stages
NEW_SYMBOLS = ['pcp_object_augment_boxes', 'pcp_object_augment_points', 'pcp_object_augment_points_workspace_bytes', 'pcp_frame_extent',
               'pcp_frame_extent_workspace_bytes', 'pcp_object_augment_drop_boxes']


def _aug(name, **kw):
    return DeviceWorldAugmentor(META['cases'][name]['cfg'], META['pc_range'], object_stages=True, **kw)


def test_default_still_skips_and_opt_in_queues(caplog):
    cfg = META['cases']['full']['cfg'] + [{'NAME': 'random_local_pyramid_aug'}, {'NAME': 'random_image_flip'}]
    with caplog.at_level(logging.INFO):
        off = DeviceWorldAugmentor(cfg, META['pc_range'])
    assert [n for n, _ in off.queue] == ['random_world_rotation', 'random_world_flip'] and not off.has_object_stages
    assert off.steps == [{'kind': 'world', 'q': [0, 1], 'stages': off.stages}]          # one world step carrying every stage
    assert set(off.skipped) == set(oar.OBJECT_NAMES) | {'random_local_pyramid_aug', 'random_image_flip'}
    assert sum('skipped' in r.message for r in caplog.records) == len(off.skipped)
    on = DeviceWorldAugmentor(cfg, META['pc_range'], object_stages=True)
    assert [n for n, _ in on.queue] == [c['NAME'] for c in META['cases']['full']['cfg']]
    assert on.skipped == ['random_local_pyramid_aug', 'random_image_flip']
    assert [s['kind'] for s in on.steps] == ['world', 'local', 'wdrop', 'world'] and on.splits == []
    assert on.steps[1]['stages'] == [1, 2, 3, 5, 4, 6, 8] and on.steps[2]['stages'] == [11, 13]
    # without object entries in the list the switch changes nothing
    a, b = DeviceWorldAugmentor(cfg[:1] + cfg[-3:-2], META['pc_range']), DeviceWorldAugmentor(cfg[:1] + cfg[-3:-2], META['pc_range'], object_stages=True)
    assert a.queue == b.queue and a.stages == b.stages and a.steps == b.steps and [s['kind'] for s in b.steps] == ['world']
    pa, pb = a.draw(3, np.random.RandomState(4)), b.draw(3, np.random.RandomState(4))
    assert all(np.array_equal(pa[k], pb[k]) for k in pa) and set(pa) == set(pb)


def test_a_count_changing_stage_in_front_of_an_object_stage_splits_the_draws():
    lst = META['cases']['w10']['cfg']
    aug = DeviceWorldAugmentor([lst[3], lst[0], lst[1]], META['pc_range'], object_stages=True)
    assert aug.splits == [1] and [s['kind'] for s in aug.steps] == ['wdrop', 'local']
    assert _aug('w10').splits == []                              # the dropout is last: the box counts stay a host fact


@pytest.mark.parametrize('name', CASES)
def test_draw_reproduces_the_reference_draws(name):
    c = oar.case_arrays(D, name)
    m = META['cases'][name]
    aug = _aug(name)
    p = aug.draw(len(META['sizes']), np.random.RandomState(m['seed']), n_boxes=META['n_boxes'])
    for b in range(len(META['sizes'])):
        want = c['draws'][c['draws_off'][b]:c['draws_off'][b + 1]]
        got = oar.flat_draws(m['cfg'], p, b)
        assert np.array_equal(got, want), (name, b)
    assert np.array_equal(p['flip_x'], c['flip_x'].astype(bool)) and np.array_equal(p['flip_y'], c['flip_y'].astype(bool))
    with pytest.raises(ValueError, match='n_boxes'):
        aug.draw(3, np.random.RandomState(0))


def test_scalar_angle_and_early_return_rules():
    assert obj.sub_stages('random_local_rotation', {'LOCAL_ROT_ANGLE': 0.3}) == [(lib.OBJ_ROTATE, -0.3, 0.3)]
    assert obj.sub_stages('random_local_rotation', {'LOCAL_ROT_ANGLE': [-0.2, 0.4]}) == [(lib.OBJ_ROTATE, -0.2, 0.4)]
    assert obj.sub_stages('random_local_scaling', {'LOCAL_SCALE_RANGE': [1.0, 1.0005]}) == []
    rng = np.random.RandomState(1)
    state = rng.get_state()[1].copy()
    assert obj.draw_entry('random_local_scaling', {'LOCAL_SCALE_RANGE': [1.0, 1.0005]}, 5, rng).shape == (0, 5)
    assert np.array_equal(rng.get_state()[1], state)             # nothing drawn
    aug = _aug('lscale_skip')
    assert aug.steps[0]['stages'] == [lib.OBJ_ROTATE]


def test_refusals_come_before_any_launch():
    pts = torch.zeros((4, 5))
    with pytest.raises(ValueError, match='velocity'):
        obj.local_stages(pts, torch.zeros((1, 3, 10)), [lib.OBJ_ROTATE], [np.ones((1, 0))])
    with pytest.raises(ValueError, match=str(lib.OBJ_MAX_BOXES)):
        obj.local_stages(pts, torch.zeros((1, lib.OBJ_MAX_BOXES + 1, 8)), [lib.OBJ_SCALE], [np.ones((1, 0))])
    with pytest.raises(ValueError, match='float32'):
        obj.local_stages(pts.double(), torch.zeros((1, 3, 8)), [lib.OBJ_SCALE], [np.ones((1, 0))])
    with pytest.raises(ValueError, match='float32'):
        obj.world_dropout(pts, torch.zeros((1, 3, 8), dtype=torch.float64), None, lib.OBJ_WORLD_DROP_TOP, [0.1])
    with pytest.raises(ValueError, match='sub-stages'):
        obj.descriptor([1] * (lib.OBJ_MAX_STAGES + 1), 1)
    with pytest.raises(lib.PcpError):
        obj.local_stages(pts, torch.zeros((1, 3, 8)), [lib.OBJ_SCALE], [np.ones((1, 0))])        # CPU tensors: no fallback


def test_symbols_and_constants_agree_with_the_header():
    header = open(os.path.join(REPO, 'include', 'pcp_hip_train.h')).read()
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.SYMBOLS and hasattr(L, name) and re.search(r'\b%s\s*\(' % name, header), name
    for key in re.findall(r'#define PCP_(OBJ_[A-Z_]+) (\d+)', header):
        assert getattr(lib, key[0]) == int(key[1]), key
    st = lib.ObjectAug()
    assert len(st.stage) == lib.OBJ_MAX_STAGES
    # refused in the library before any launch (no GPU is touched)
    a = obj.descriptor([lib.OBJ_WORLD_DROP_TOP, lib.OBJ_SCALE], 1)
    assert L.pcp_object_augment_points(a, None, None, 0, None, None, 0, 5, None, None, None, 0, None) == 1      # PCP_ERR_ARG
    a = obj.descriptor([lib.OBJ_SCALE], 1)
    assert L.pcp_object_augment_points(a, None, None, lib.OBJ_MAX_BOXES + 1, None, None, 0, 5, None, None, None, 0, None) == 4   # PCP_ERR_UNSUPPORTED
    assert L.pcp_frame_extent(None, 0, 5, 0, 2, None, None, 0, None) == 1


@pytest.mark.parametrize('name', OBJECT_ONLY)
def test_numpy_restatement_matches_the_fixture(name):
    c = oar.case_arrays(D, name)
    m = META['cases'][name]
    off = np.cumsum([0] + META['sizes'])
    worst = 0.0
    for b in range(len(META['sizes'])):
        pts, gt = c['points'][off[b]:off[b + 1], 1:], c['gt_boxes'][b, :META['n_boxes'][b]]
        draws = c['draws'][c['draws_off'][b]:c['draws_off'][b + 1]]
        lst = m['cfg']
        steps, _, _ = oar.steps_of(lst, draws, gt.shape[0])
        p, g, ids = oar.restate_frame(pts, gt, steps)
        want_ids = c['kept_rows'][(c['kept_rows'] >= off[b]) & (c['kept_rows'] < off[b + 1])] - off[b]
        assert np.array_equal(ids, want_ids)
        want = c['points_out'][c['points_out'][:, 0] == b][:, 1:]
        assert np.array_equal(p[:, 3:], want[:, 3:])
        g[:, 6] = oar.limit_period(g[:, 6])
        want_g = c['gt_boxes_out'][b, :m['boxes_kept'][b]]
        assert g.shape == want_g.shape
        if all(s[0] <= oar.TRANSLATE_Z or s[0] >= oar.DROP_TOP for s in steps):
            assert np.array_equal(p[:, :3], want[:, :3]) and np.array_equal(g, want_g)
        err = max(float(np.abs(p[:, :3] - want[:, :3]).max(initial=0.0)), float(np.abs(g - want_g).max(initial=0.0)))
        worst = max(worst, err)
        assert err <= oar.COORD_TOL, err
    print('%s: max |restatement - fixture| = %.3g (bound %.3g)' % (name, worst, oar.COORD_TOL))


def test_the_whole_plan_is_checked_before_its_first_launch():
    """a world rotation in front of a local rotation on 10-column boxes: the refusal arrives although the world step comes first (on these
    CPU tensors a launched world step would have raised PcpError instead)"""
    lst = META['cases']['full']['cfg']
    aug = DeviceWorldAugmentor([lst[0], lst[2]], META['pc_range'], object_stages=True)
    assert [s['kind'] for s in aug.steps] == ['world', 'local']
    bd = {'points': torch.zeros((4, 5)), 'gt_boxes': torch.zeros((1, 3, 10)), 'batch_size': 1}
    p = aug.draw(1, np.random.RandomState(0), n_boxes=[0])
    with pytest.raises(ValueError, match='velocity'):
        aug.apply(bd, p)
    bd = {'points': torch.zeros((4, 5), dtype=torch.float64), 'gt_boxes': torch.zeros((1, 3, 8)), 'batch_size': 1}
    with pytest.raises(ValueError, match='float32'):
        aug.apply(bd, p)
    bd = {'points': torch.zeros((4, 5)), 'gt_boxes': torch.zeros((1, lib.OBJ_MAX_BOXES + 1, 8)), 'batch_size': 1}
    with pytest.raises(ValueError, match=str(lib.OBJ_MAX_BOXES)):
        aug.apply(bd, p)


def test_gt_sampling_behind_an_object_stage_is_refused():
    lst = META['cases']['w10']['cfg']
    sampler = object()
    with pytest.raises(ValueError, match='gt_sampling behind random_local_translation'):
        DeviceWorldAugmentor([lst[0], {'NAME': 'gt_sampling'}], META['pc_range'], object_stages=True, gt_sampler=sampler)
    aug = DeviceWorldAugmentor([{'NAME': 'gt_sampling'}, lst[0]], META['pc_range'], object_stages=True, gt_sampler=sampler)
    assert aug.splits == [1] and [s['kind'] for s in aug.steps] == ['gt', 'local']
    DeviceWorldAugmentor([lst[0], {'NAME': 'gt_sampling'}], META['pc_range'], object_stages=True)        # no sampler: the entry is skipped


def test_the_synthetic_loader_hands_the_host_box_counts_over():
    from pcdet.datasets import SyntheticV2XDataset
    items = [{'points': np.zeros((3, 5), np.float32), 'frame_id': i, 'metadata': {}, 'gt_boxes': np.ones((k, 8), np.float32)} for i, k in enumerate((2, 0, 5))]
    batch = SyntheticV2XDataset.collate_batch(items)
    assert batch['num_gt_boxes'] == [2, 0, 5] and batch['gt_boxes'].shape == (3, 5, 8)
    assert DeviceWorldAugmentor.box_counts(batch) == [2, 0, 5]       # taken as they are: nothing is read from the device
