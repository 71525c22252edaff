"""Host side of the device world augmentation (pcp_amd/augment.py), no GPU: the parameters DeviceWorldAugmentor.draw() draws equal the
ones the reference drew (tests/golden/g26_augment.npz, made by tests/golden/make_golden_augment.py from the reference's own functions),
the config is parsed like DataAugmentor.__init__ parses it, se3_from_ego follows the reference, and the numpy restatement of the
kernels' arithmetic (tests/augment_refs.py, the second reference of the GPU tests) stays inside the bounds the GPU tests use."""
import logging

import numpy as np
import pytest

import augment_refs as ar
from pcp_amd import lib
from pcp_amd.augment import DeviceWorldAugmentor, augment_se3_from_ego

D, META = ar.load_fixture()
CASES = [c for c in META['cases'] if c != 'empty']


def augmentor_of(name, **kw):
    m = META['cases'][name]
    return DeviceWorldAugmentor(m['cfg'], META['pc_range'], layout='nusc_map' if m['hd_map'] else 'car', **kw)


def test_conditioning_recorded_in_the_fixture():
    lim = np.asarray(META['pc_range'])
    assert META['conditioning']['margin'] == 1e-4 and META['largest_coord'] <= ar.COORD_MAX
    for name in CASES:
        c = ar.case_arrays(D, name)
        p = c['points_out'][:, 1:4].astype(np.float64)
        for a in range(3):
            assert (np.abs(p[:, a] - lim[a]) >= 1e-4).all() and (np.abs(p[:, a] - lim[a + 3]) >= 1e-4).all()
        assert (np.abs(np.abs(c['gt_boxes_out'][..., 6].astype(np.float64)) - np.pi) >= 1e-4).all()
    # the flips of one case cover none, x only and both; points fall outside on every side
    c = ar.case_arrays(D, 'w7')
    assert {(int(a), int(b)) for a, b in zip(c['flip_x'], c['flip_y'])} >= {(0, 0), (1, 0), (1, 1)}
    c = ar.case_arrays(D, 'w13')
    p = c['points_out'][:, 1:4]
    for a in range(3):
        assert (p[:, a] < lim[a]).any() and (p[:, a] >= lim[a + 3]).any()
    assert (c['points'][:, 14 - 3] > 0).any() and (c['points'][:, 14 - 3] == 0).any()
    assert 0 in META['cases']['w6']['sizes'] and D['empty/points'].shape[0] == 0
    assert [sum(META['cases'][n]['sizes']) for n in ('w6', 'w7', 'w12')] == [ar.TILE_ROWS - 1, ar.TILE_ROWS, ar.TILE_ROWS + 1]
    assert ar.TILE_ROWS == lib.AUG_TILE_ROWS and sum(META['cases']['w13']['sizes']) % ar.TILE_ROWS not in (0, 1, ar.TILE_ROWS - 1)


@pytest.mark.parametrize('name', ['w6', 'w12', 'w13', 'w7d', 'w7'])
def test_draw_reproduces_the_parameters_the_reference_drew(name):
    """two list orders (w12: flip, rotation, scaling, translation; w13: translation, scaling, rotation, flip y x) and one entry disabled (w7d)"""
    m = META['cases'][name]
    c = ar.case_arrays(D, name)
    p = augmentor_of(name).draw(len(m['sizes']), np.random.RandomState(m['seed']))
    assert np.array_equal(p['flip_x'], c['flip_x'].astype(bool)) and np.array_equal(p['flip_y'], c['flip_y'].astype(bool))
    assert np.array_equal(p['noise_rot'], c['noise_rot']) and np.array_equal(p['noise_scale'], c['noise_scale'])
    assert np.array_equal(p['noise_translate'], c['noise_translate']) and p['noise_translate'].dtype == np.float32


def test_config_parsing(caplog):
    cfg = {'DISABLE_AUG_LIST': ['random_world_scaling'],
           'AUG_CONFIG_LIST': [{'NAME': 'gt_sampling', 'DB_INFO_PATH': ['x.pkl']}, {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['y', 'x']},
                               {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': 0.3}, {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.9, 1.1]},
                               {'NAME': 'random_local_rotation', 'LOCAL_ROT_ANGLE': 0.1},
                               {'NAME': 'random_world_translation', 'NOISE_TRANSLATE_STD': [0.5, 0.5, 0.5]}]}
    with caplog.at_level(logging.INFO):
        aug = DeviceWorldAugmentor(cfg, [-1, -1, -1, 1, 1, 1], data_processor=[{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}])
    assert [n for n, _ in aug.queue] == ['random_world_flip', 'random_world_rotation', 'random_world_translation']
    assert aug.stages == [lib.AUG_FLIP_Y, lib.AUG_FLIP_X, lib.AUG_ROTATE, lib.AUG_TRANSLATE]
    assert aug.skipped == ['gt_sampling', 'random_local_rotation'] and aug.filter and not aug.hd_map
    lines = [r.getMessage() for r in caplog.records]
    assert sum('gt_sampling' in x for x in lines) == 1 and sum('random_local_rotation' in x for x in lines) == 1
    assert aug.rot_range(aug.queue[1][1]) == [-0.3, 0.3]                     # a scalar WORLD_ROT_ANGLE means [-a, a]
    p = aug.draw(64, np.random.RandomState(0))
    assert (np.abs(p['noise_rot']) <= 0.3).all() and (p['noise_scale'] == 1.0).all() and p['flip_x'].any() and not p['flip_x'].all()
    # the bare list form (no DISABLE_AUG_LIST), no range mask in the processor list
    bare = DeviceWorldAugmentor(cfg['AUG_CONFIG_LIST'][1:4], [-1, -1, -1, 1, 1, 1], layout='nusc_map', data_processor=[{'NAME': 'shuffle_points'}])
    assert bare.stages == [lib.AUG_FLIP_Y, lib.AUG_FLIP_X, lib.AUG_ROTATE, lib.AUG_SCALE] and not bare.filter and bare.hd_map
    # the project's own V2X-Sim dataset config carries the list the augmentor reads
    from pcdet.config import EasyDict, cfg_from_yaml_file
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'practical-collab-perception_amd', 'tools', 'cfgs', 'dataset_configs')
    dc = cfg_from_yaml_file(os.path.join(root, '_v2x_sim_common.yaml'), EasyDict())
    a = DeviceWorldAugmentor.from_dataset_cfg(dc, layout='disco')
    assert a.stages == [lib.AUG_FLIP_X, lib.AUG_FLIP_Y, lib.AUG_ROTATE, lib.AUG_SCALE] and a.filter


@pytest.mark.parametrize('name', ['w6', 'w13'])
def test_se3_from_ego_matches_the_reference(name):
    c = ar.case_arrays(D, name)
    aug = augmentor_of(name)
    p = ar.params_of(c)
    worst = 0.0
    for b in range(c['se3'].shape[0]):
        got = augment_se3_from_ego({int(k): c['se3'][b, i] for i, k in enumerate(c['se3_keys'])}, aug.stages, p, b)
        for i, k in enumerate(c['se3_keys']):
            worst = max(worst, float(np.abs(got[int(k)] - c['se3_out'][b, i]).max()))
    print('%s: max |se3_from_ego - reference| = %.3g' % (name, worst))
    assert worst <= 1e-12
    assert any(np.abs(c['se3_out'][b] - c['se3'][b]).max() > 1e-3 for b in range(c['se3'].shape[0]))


@pytest.mark.parametrize('name', CASES)
def test_numpy_restatement_matches_the_fixture(name):
    m = META['cases'][name]
    c = ar.case_arrays(D, name)
    aug = augmentor_of(name)
    stages = ar.stages_of(m['cfg']['AUG_CONFIG_LIST'])
    disabled = m['cfg']['DISABLE_AUG_LIST']
    stages = ar.stages_of([x for x in m['cfg']['AUG_CONFIG_LIST'] if x['NAME'] not in disabled])
    assert stages == aug.stages
    table = aug.table(ar.params_of(c))
    out, keep = ar.restate_points(c['points'], table, stages, m['hd_map'], META['pc_range'])
    assert np.array_equal(keep, c['mask']) and [int(keep[c['points'][:, 0] == b].sum()) for b in range(len(m['sizes']))] == m['kept']
    S = out.shape[1]
    angle_cols = ([10] if m['hd_map'] else []) + ([9] if S >= 14 else [])
    same = [k for k in range(S) if k not in (1, 2, 3) and k not in angle_cols]
    assert np.array_equal(out[:, same].view(np.uint32), c['points_out'][:, same].view(np.uint32))
    e_xyz = float(np.abs(out[:, 1:4].astype(np.float64) - c['points_out'][:, 1:4]).max())
    e_ang = max([float(np.abs(out[:, k].astype(np.float64) - c['points_out'][:, k]).max()) for k in angle_cols] or [0.0])
    gt = ar.restate_boxes(c['gt_boxes'], table, stages)
    W = gt.shape[2]
    lin = [0, 1, 2, 3, 4, 5] + ([7, 8] if W == 10 else [])
    e_box = float(np.abs(gt[..., lin].astype(np.float64) - c['gt_boxes_out'][..., lin]).max())
    e_head = float(np.abs(gt[..., 6].astype(np.float64) - c['gt_boxes_out'][..., 6]).max())
    pad = c['gt_boxes'][..., W - 1] == 0
    assert pad.any() and np.array_equal(gt[pad].view(np.uint32), c['gt_boxes'][pad].view(np.uint32))
    assert np.array_equal(gt[..., W - 1], c['gt_boxes'][..., W - 1])
    e_tf = 0.0
    if 'instances_tf' in c:
        tf = ar.restate_tf(c['instances_tf'], c['gt_boxes'], table, stages)
        e_tf = float(np.abs(tf.astype(np.float64) - c['instances_tf_out']).max())
        assert np.array_equal(tf[pad].view(np.uint32), c['instances_tf'][pad].view(np.uint32))
    print('%s: xyz %.3g (bound %.3g), point angles %.3g, box %.3g, heading %.3g (bound %.3g), tf %.3g (bound %.3g)'
          % (name, e_xyz, ar.COORD_TOL, e_ang, e_box, e_head, ar.ANGLE_TOL, e_tf, ar.tf_tol(META['largest_tf'])))
    assert e_xyz <= ar.COORD_TOL and e_box <= ar.COORD_TOL and e_ang <= ar.ANGLE_TOL and e_head <= ar.ANGLE_TOL
    assert e_tf <= ar.tf_tol(META['largest_tf'])


def test_host_refusals_need_no_device():
    """widths the kernels do not take are refused on the host with the limit in the message, before any launch: the C entry points
    validate their arguments without touching a device, and the tensor checks of the wrapper come first"""
    import ctypes
    L = lib.load()
    a = lib.WorldAug()
    a.n_stages, a.batch = 0, 2
    assert L.pcp_world_augment_points(ctypes.byref(a), ctypes.c_void_p(256), ctypes.c_void_p(256), 10, 3, ctypes.c_void_p(256), None, None, 0, None) != 0
    assert L.pcp_world_augment_points(ctypes.byref(a), ctypes.c_void_p(256), ctypes.c_void_p(256), 10, 16, ctypes.c_void_p(256), None, None, 0, None) != 0
    assert L.pcp_world_augment_boxes(ctypes.byref(a), ctypes.c_void_p(256), ctypes.c_void_p(256), 4, 9, None, 0, 0, None) != 0
    assert L.pcp_world_augment_boxes(ctypes.byref(a), ctypes.c_void_p(256), ctypes.c_void_p(256), 4, 8, ctypes.c_void_p(256), 3, 5, None) != 0
    a.n_stages = 9
    assert L.pcp_world_augment_boxes(ctypes.byref(a), ctypes.c_void_p(256), ctypes.c_void_p(256), 4, 8, None, 0, 0, None) != 0
    assert L.pcp_world_augment_points_workspace_bytes(0) > 0 and L.pcp_world_augment_points_workspace_bytes(513) >= 8
    # no CPU path
    import torch
    aug = augmentor_of('w7')
    with pytest.raises((lib.PcpError, RuntimeError)):
        aug.augment_points(torch.zeros(4, 8), torch.zeros(3, lib.AUG_TABLE_STRIDE), 3)
