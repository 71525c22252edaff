"""nuScenes PointPillar-Jr models, CPU side: the two configs build through build_network (SCConvBackbone2dStride4 is in the
registry, CenterHead takes the vel / iou branches) with the reference's parameter tree -- key names and shapes recorded from the
reference's own modules by tests/golden/make_golden_nusc.py -- and the SC backbones refuse training mode."""
import os

import numpy as np
import pytest
import torch

from helpers import load_golden

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CFGS = os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'nuscenes_models')


def _build_from_yaml(name):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    cfg = cfg_from_yaml_file(os.path.join(CFGS, name), EasyDict())
    vs = [p['VOXEL_SIZE'] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(cfg.DATA_CONFIG.POINT_FEATURE_ENCODING.used_feature_list))
    return cfg, ds, build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)


def _shapes(model):
    return {k: [int(x) for x in v.shape] for k, v in model.state_dict().items()}


@pytest.mark.parametrize('yaml_name,case', [('pointpillar_jr_nomap.yaml', 'nomap'), ('pointpillar_jr_withmap.yaml', 'withmap')])
def test_pointpillar_jr_builds_with_the_reference_parameter_tree(yaml_name, case):
    cfg, ds, model = _build_from_yaml(yaml_name)
    g = load_golden('g20_nusc_mini.npz')
    want = g['meta']['cases'][case]['state_shapes']
    got = _shapes(model)
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:20]
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    # the real geometry: 512 x 512 pillars of 0.2 m, ten classes in six heads, 7 / 12 point columns
    assert list(ds.grid_size) == [512, 512, 1]
    assert len(cfg.CLASS_NAMES) == 10 and len(model.dense_head.heads_list) == 6
    assert ds.point_feature_encoder.num_point_features == (7 if case == 'nomap' else 12)
    assert type(model.backbone_2d).__name__ == 'SCConvBackbone2dStride4' and model.backbone_2d.num_bev_features == 384


def test_pointpillar_jr_quirks_of_the_reference():
    """conv_out keeps nn.BatchNorm2d's default eps (1e-5) while every other BatchNorm of the backbone has 1e-3; k2 index 0 is the pool"""
    _cfg, _ds, model = _build_from_yaml('pointpillar_jr_nomap.yaml')
    bb = model.backbone_2d
    assert bb.conv_out[1].eps == 1e-5
    eps = {m.eps for n, m in bb.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and not n.startswith('conv_out')}
    assert eps == {1e-3}
    assert isinstance(bb.stem[1].scconv.k2[0], torch.nn.AvgPool2d)
    sd = bb.state_dict()
    for k in ('stem.1.conv1_a.weight', 'stem.1.scconv.k2.1.weight', 'main_pass.4.weight', 'conv_out.1.running_var'):
        assert k in sd, k
    assert tuple(sd['main_pass.4.weight'].shape) == (256, 256, 2, 2)


def test_meta_builder_knows_the_nuscenes_layouts():
    from pcdet.models import build_network_from_meta
    g = load_golden('g20_nusc_mini.npz')
    for case in ('nomap', 'withmap'):
        model = build_network_from_meta(g['meta']['cases'][case])
        assert _shapes(model) == g['meta']['cases'][case]['state_shapes']
        assert model.vfe.num_raw_point_features == (5 if case == 'nomap' else 10)


def test_sc_conv_backbone_stride1_parameter_tree():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d import __all__ as registry
    g = load_golden('g20_nusc_mini.npz')
    m = g['meta']['cases']['stride1']
    bb = registry['SCConvBackbone2dStride1'](EasyDict(m['cfg']), m['input_channels'])
    assert _shapes(bb) == m['state_shapes']
    assert bb.num_bev_features == m['cfg']['NUM_BEV_FEATURES']


def test_sc_backbone_training_mode_is_refused():
    _cfg, _ds, model = _build_from_yaml('pointpillar_jr_nomap.yaml')
    bb = model.backbone_2d
    bb.train()
    with pytest.raises(NotImplementedError):
        bb({'spatial_features': torch.zeros(1, 64, 8, 8)})


def test_nusc_cloud_layouts():
    from pcp_amd import synth
    a = synth.nusc_cloud(0, 100)
    b = synth.nusc_cloud(0, 100, with_map=True)
    assert a.shape == (100, 7) and b.shape == (100, 12)
    assert np.array_equal(a[:, :5], b[:, :5]) and np.array_equal(a[:, 5:], b[:, 10:])
    assert a[:, 2].min() >= -5.0 and a[:, 2].max() < 3.0
