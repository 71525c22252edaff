"""v2x_second_car / v2x_second_rsu, CPU side: the two YAMLs resolve to the reference's MODEL sections and build the reference's parameter
trees (both recorded from the reference's own config loader and modules by tests/golden/make_golden_second_corr.py), the seeded inputs of
the 256-channel point-head kernel tests keep their dynamic-foreground verdicts clear of the threshold in float64, and the new fixture
satisfies its conditioning caps and the size limit."""
import os

import numpy as np
import pytest
import torch

import second_corr_refs as R
from helpers import load_golden
from test_nusc_corr_cpu import _flatten, _plain

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CFGS = os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models')
FIXTURE = 'g30_second_corr_module.npz'
CASES = {32: 'v2x_second_car.yaml', 64: 'v2x_second_rsu.yaml'}


@pytest.fixture(scope='module')
def golden():
    return load_golden(FIXTURE)


def _build(hidden):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    cfg = cfg_from_yaml_file(os.path.join(CFGS, CASES[hidden]), EasyDict())
    vs = [p['VOXEL_SIZE'] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(cfg.DATA_CONFIG.POINT_FEATURE_ENCODING.used_feature_list))
    return cfg, ds, build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)


@pytest.mark.parametrize('hidden', sorted(CASES))
def test_yaml_resolves_to_the_reference_model_section(golden, hidden):
    cfg, ds, _model = _build(hidden)
    meta = golden['meta']['cases'][str(hidden)]
    assert meta['yaml'] == CASES[hidden]
    want, got = _flatten(meta['ref_model']), _flatten(_plain(cfg.MODEL))
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got['CORRECTOR.POINT_HEAD_HIDDEN_CHANNELS'] == got['CORRECTOR.OBJ_HEAD_HIDDEN_CHANNELS'] == [hidden]
    assert got['CORRECTOR.BEV_IMAGE_STRIDE'] == 8 and got['VFE.NUM_POINT_FEATURES'] == 5
    # car writes the exchange database, rsu does not; both name the SECOND one
    assert got['CORRECTOR.GENERATING_EXCHANGE_DATA'] is (hidden == 32) and got['DENSE_HEAD.GENERATING_EXCHANGE_DATA'] is (hidden == 32)
    assert got['CORRECTOR.DATABASE_EXCHANGE_DATA'].endswith('exchange_database_second')
    assert got['DENSE_HEAD.DATABASE_EXCHANGE_DATA'].endswith('exchange_database_second')
    assert list(cfg.CLASS_NAMES) == meta['ref_class_names']
    assert [float(v) for v in cfg.DATA_CONFIG.POINT_CLOUD_RANGE] == meta['ref_pc_range']
    if hidden == 32:
        # the two keys car's YAML overrides itself (rsu's YAML sets neither: its range is the dataset config's)
        assert meta['ref_pc_range'] == [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
        assert cfg.DATA_CONFIG.MINI_TRAINVAL_STRIDE == meta['ref_mini_trainval_stride'] == 1
    assert ds.point_feature_encoder.num_point_features == meta['ref_point_features']
    assert cfg.OPTIMIZATION.OPTIMIZER == 'adam_onecycle' and cfg.OPTIMIZATION.LR == 0.00051 and cfg.OPTIMIZATION.NUM_EPOCHS == 20


@pytest.mark.parametrize('hidden', sorted(CASES))
def test_state_dict_is_the_reference_parameter_tree(golden, hidden):
    _cfg, _ds, model = _build(hidden)
    want = golden['meta']['cases'][str(hidden)]['ref_state_shapes']
    got = {k: [int(x) for x in v.shape] for k, v in model.state_dict().items()}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:20]
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert any(k.startswith('corrector.object_head.') for k in got)
    assert got['corrector.point_head.local_feat_predictor.0.weight'] == [hidden, 256]
    assert got['corrector.conv_input.0.weight'] == [256, 256, 3, 3] and got['corrector.conv_weightor.0.0.weight'] == [512, 512, 3, 3]
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelResBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                             'HunterJr', 'CenterHead']
    # the corrector's own tree is the one the module fixture was generated with
    sub = {k[len('corrector.'):]: v for k, v in got.items() if k.startswith('corrector.')}
    assert sub == golden['meta']['cases'][str(hidden)]['state_shapes']


@pytest.mark.parametrize('hidden', R.HIDDEN)
@pytest.mark.parametrize('n', R.NS)
def test_kernel_inputs_keep_their_verdicts_in_float64(hidden, n):
    """the cases of tests/test_gpu_second_corr.py at C = 256: sampled rows by oracle/bev.py's sampler, MLP and heads in float64"""
    c = R.case(256, hidden, n)
    assert c['bev'].shape == (2, 8, 8, 256) and c['points'].shape == (n, 13) and c['w1'].shape == (hidden, 256)
    pf = R.oracle_pf(c)
    none = c['points'][:, 0] < 0
    assert not pf[torch.from_numpy(none)].any()                              # rows of no frame sample nothing
    if n >= 31:
        assert none[4::7].all() and int(none.sum()) == len(range(4, n, 7))
        outside = (np.abs(c['points'][:, 1:3]) > 3.2).any(1)
        assert 0.05 < float(outside.mean()) < 0.5
    head8 = R.head8_torch(c, pf)
    assert R.verdict_margin(head8) > 1e-3
    if n >= 31:
        share = float(R.dynamic_rows(head8).float().mean())
        assert 0.0 < share < 1.0, share


def test_module_fixture_satisfies_its_conditioning_caps(golden):
    g = golden
    n = g['points'].shape[0]
    assert g['points'].shape == (600, 13)
    x, y = g['points'][:, 1], g['points'][:, 2]
    for side in (x < -4.8, x > 4.8, y < -4.8, y > 4.8):
        assert side.any()
    assert g['meta']['num_bev_features'] == 256 and g['meta']['map']['shape'] == [2, 256, 12, 12]
    assert g['meta']['voxel_size'][:2] == [0.1, 0.1]
    for hidden in sorted(CASES):
        t = 'h%d_' % hidden
        meta = g['meta']['cases'][str(hidden)]
        assert meta['corrector']['POINT_HEAD_HIDDEN_CHANNELS'] == [hidden] and meta['corrector']['BEV_IMAGE_STRIDE'] == 8
        assert g[t + 'spatial_features_2d'].shape == (2, 256, 12, 12) and g[t + 'head8'].shape == (n, 8)
        dyn = g[t + 'dyn'].astype(bool)
        share = float(dyn.mean())
        assert 0.05 <= share <= 0.5 and abs(share - meta['dyn_share']) < 1e-6
        moved = np.abs(g[t + 'points_after'] - g['points']).max(1) > 0
        assert np.array_equal(moved, dyn)
        cls = torch.from_numpy(g[t + 'head8'][:, :3]).double()
        p = torch.sigmoid(cls)
        two = torch.topk(cls, 2, dim=1)[0]
        assert float((p.max(1)[0] - 0.3).abs().min()) >= 1e-3 and float((two[:, 0] - two[:, 1]).min()) > 2e-4
        assert np.array_equal(((p.argmax(1) == 2) & (p.max(1)[0] > 0.3)).numpy(), dyn)
        # no corrected row within 2.5e-4 pixel (0.8 m) of a pixel boundary
        cpix = (g[t + 'points_after'][dyn, 1:3].astype(np.float64) + 4.8) / 0.8
        assert float(np.abs(cpix - np.round(cpix)).min()) >= 2.5e-4


def test_new_fixtures_are_within_the_size_limit():
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', FIXTURE)) <= 1 << 20


@pytest.mark.parametrize('hidden', sorted(CASES))
def test_training_is_refused(hidden):
    _cfg, _ds, model = _build(hidden)
    with pytest.raises(NotImplementedError, match='inference only'):
        model.train()
    model.eval()
