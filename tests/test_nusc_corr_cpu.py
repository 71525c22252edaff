"""pointpillar_jr_corr_withmap, CPU side: the YAML resolves to the reference's MODEL section and builds the reference's parameter tree (both
recorded from the reference's own config loader and modules by tests/golden/make_golden_nusc_corr.py), the g24_corr fixtures satisfy their
own conditioning caps, and training the nuScenes corrector is refused with a message that names the limit."""
import os

import numpy as np
import pytest
import torch

from helpers import load_golden

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
YAML = os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_corr_withmap.yaml')


def _build():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    cfg = cfg_from_yaml_file(YAML, EasyDict())
    vs = [p['VOXEL_SIZE'] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(cfg.DATA_CONFIG.POINT_FEATURE_ENCODING.used_feature_list))
    return cfg, ds, build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)


def _plain(d):
    if isinstance(d, dict):
        return {k: _plain(v) for k, v in d.items()}
    if isinstance(d, (list, tuple)):
        return [_plain(v) for v in d]
    return d


def _flatten(d, prefix=''):
    """nested dicts -> {dotted name: value}; lists are values.  _BASE_CONFIG_ is the loader's include directive (this project's YAML names
    the shared trunk file with it), not a setting"""
    out = {}
    for k, v in d.items():
        if k == '_BASE_CONFIG_':
            continue
        if isinstance(v, dict):
            out.update(_flatten(v, prefix + k + '.'))
        else:
            out[prefix + k] = v
    return out


def test_yaml_resolves_to_the_reference_model_section():
    cfg, ds, _model = _build()
    meta = load_golden('g24_corr_module.npz')['meta']
    want, got = _flatten(meta['ref_model']), _flatten(_plain(cfg.MODEL))
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got['CORRECTOR.NAME'] == 'HunterJr' and got['CORRECTOR.POINT_HEAD_HIDDEN_CHANNELS'] == [64]
    assert list(cfg.CLASS_NAMES) == meta['ref_class_names']
    # 13-column clouds: the batch index + 12 point features, of which the VFE reads the first 10
    assert ds.point_feature_encoder.num_point_features == meta['ref_point_features'] == 12
    assert cfg.MODEL.VFE.NUM_RAW_POINT_FEATURES == 10


def test_state_dict_is_the_reference_parameter_tree():
    _cfg, _ds, model = _build()
    want = load_golden('g24_corr_module.npz')['meta']['ref_state_shapes']
    got = {k: [int(x) for x in v.shape] for k, v in model.state_dict().items()}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:20]
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert any(k.startswith('corrector.object_head.') for k in got)           # built at construction, as in the reference
    assert got['corrector.point_head.local_feat_predictor.0.weight'] == [64, 384]
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFE', 'PointPillarScatter', 'SCConvBackbone2dStride4', 'HunterJr',
                                                             'CenterHead']


def test_meta_builder_builds_the_fixture_models():
    from pcdet.models import build_network_from_meta
    for name in ('g24_corr_mini.npz', 'g24_corr_full.npz'):
        meta = load_golden(name)['meta']['cases']['corr']
        model = build_network_from_meta(meta)
        assert {k: [int(x) for x in v.shape] for k, v in model.state_dict().items()} == meta['state_shapes']
        for key, vals in meta['state_overrides'].items():
            assert meta['state_shapes'][key] == [len(vals)]


def test_fixtures_satisfy_their_conditioning_caps():
    g = load_golden('g24_corr_module.npz')
    n = g['points'].shape[0]
    assert g['points'].shape[1] == 13 and 550 <= n <= 650
    assert g['spatial_features_2d'].shape == (2, 384, 12, 12) and g['head8'].shape == (n, 8)
    share = float(g['dyn'].mean())
    assert 0.05 <= share <= 0.5 and abs(share - g['meta']['dyn_share']) < 1e-6
    x, y = g['points'][:, 1], g['points'][:, 2]
    for side in (x < -4.8, x > 4.8, y < -4.8, y > 4.8):
        assert side.any()                                                     # points outside the map on every side
    moved = np.abs(g['points_after'] - g['points']).max(1) > 0
    assert np.array_equal(moved, g['dyn'].astype(bool))                       # exactly the dynamic rows moved
    assert np.array_equal(g['points_after'][:, [0] + list(range(4, 13))], g['points'][:, [0] + list(range(4, 13))])
    # the verdicts are clear of the threshold and of ties
    cls = torch.from_numpy(g['head8'][:, :3]).double()
    p = torch.sigmoid(cls)
    two = torch.topk(cls, 2, dim=1)[0]
    assert float((p.max(1)[0] - 0.3).abs().min()) >= 1e-3 and float((two[:, 0] - two[:, 1]).min()) > 2e-4
    want_dyn = (p.argmax(1) == 2) & (p.max(1)[0] > 0.3)
    assert np.array_equal(want_dyn.numpy(), g['dyn'].astype(bool))
    m = load_golden('g24_corr_mini.npz')
    assert m['points'].shape[1] == 13 and m['spatial_features_2d'].shape == (2, 384, 15, 15)
    assert 0.05 <= float(m['dyn'].mean()) <= 0.5
    for b in range(2):
        assert m['corr_boxes_%d' % b].shape[0] >= 8 and m['corr_boxes_%d' % b].shape[1] == 9
    f = load_golden('g24_corr_full.npz')
    assert f['corr_boxes_0'].shape[0] >= 8 and f['corr_boxes_0'].shape[1] == 9
    assert int(np.unpackbits(f['dyn']).sum()) == f['points_after_dyn'].shape[0] >= 100
    for name in ('g24_corr_module.npz', 'g24_corr_mini.npz', 'g24_corr_full.npz', 'g24_ph32.npz'):
        assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', name)) <= 1 << 20


def test_training_the_nuscenes_corrector_is_refused():
    _cfg, _ds, model = _build()
    model.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        model({'points': torch.zeros(4, 13), 'batch_size': 1})


def test_synthetic_loader_serves_the_13_column_cloud():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    cfg = cfg_from_yaml_file(YAML, EasyDict())
    cfg.DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME = 500
    cfg.DATA_CONFIG.SYNTHETIC.NUM_FRAMES = 2
    _ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 2, False, training=False)
    batch = next(iter(loader))
    assert batch['points'].shape == (1000, 13) and batch['batch_size'] == 2
