"""Training PillarFeatureNet at any raw width, CPU side: the `fused` / `train_fused` truth table of DynamicPillarVFE, the C ABI of
pcp_pfn_train_features_w (header and ctypes binding), pointpillar_jr_withmap's VFE, the fixture g23_vfe_train_widths
(tests/golden/make_golden_nusc_vfe_train.py) and the refusal of a CPU tensor."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_golden

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
MiB = 1 << 20
# tag: (num_raw, USE_ABSLOTE_XYZ, WITH_DISTANCE, NUM_FILTERS, USE_NORM) -- the five compositions of fixture g16_pfn_variants
G16 = {'dist': (5, True, True, [64, 64], True), 'rel': (5, False, False, [64, 64], True), 'one': (4, True, False, [64], True),
       'three': (5, False, True, [32, 64, 128], True), 'wide_nonorm': (7, True, True, [48, 96], False)}


def _vfe(num_raw, use_abs=True, with_dist=False, filters=(64, 64), use_norm=True):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE
    cfg = EasyDict(NAME='DynPillarVFE', WITH_DISTANCE=with_dist, USE_ABSLOTE_XYZ=use_abs, USE_NORM=use_norm, NUM_FILTERS=list(filters))
    return DynamicPillarVFE(model_cfg=cfg, num_point_features=num_raw, voxel_size=[0.2, 0.2, 8.0], grid_size=[128, 128, 1],
                            point_cloud_range=[-12.8, -12.8, -8.0, 12.8, 12.8, 0.0])


def test_fused_and_train_fused_truth_table():
    """`fused` (which also picks the one-launch inference kernel) keeps its four widths; `train_fused` covers 3 .. 26"""
    for nr in range(3, 28):
        v = _vfe(nr)
        assert bool(v.fused) == (nr in (3, 4, 5, 11)), nr
        assert bool(v.train_fused) == (nr <= 26), nr
    for tag, (nr, use_abs, with_dist, filters, use_norm) in G16.items():
        v = _vfe(nr, use_abs, with_dist, filters, use_norm)
        assert not v.fused and not v.train_fused, tag
    # the composition of the configs without BatchNorm: one-launch inference as before, no training form
    v = _vfe(5, use_norm=False)
    assert v.fused and not v.train_fused
    g16 = load_golden('g16_pfn_variants.npz')['meta']['variants']
    assert {t: (m['num_raw'], m['use_absolute_xyz'], m['with_distance'], m['vfe_filters'], m['use_norm']) for t, m in g16.items()} == G16


def test_widths_above_the_limit_are_refused_with_the_limit_in_the_message():
    v = _vfe(27).train()
    with pytest.raises(NotImplementedError, match='at most 26 raw point features'):
        v({'points': torch.zeros(4, 28), 'batch_size': 1})
    for tag, (nr, use_abs, with_dist, filters, use_norm) in G16.items():
        v = _vfe(nr, use_abs, with_dist, filters, use_norm).train()
        with pytest.raises(NotImplementedError, match='inference kernels only'):
            v({'points': torch.zeros(4, 1 + nr), 'batch_size': 1})


def test_header_declares_and_lib_binds_the_new_entry():
    import ctypes
    from pcp_amd import lib, train_ops as tops
    from pcdet.models.backbones_3d.vfe import dynamic_pillar_vfe as dpv
    hdr = open(os.path.join(REPO, 'include', 'pcp_hip_train.h')).read()
    m = re.search(r'int pcp_pfn_train_features_w\(([^;]*)\);', hdr)
    assert m, 'pcp_hip_train.h does not declare pcp_pfn_train_features_w'
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['points', 'n', 'row_stride', 'num_raw', 'fw', 'grid', 'vox_workspace', 'fbuf', 'slot_pillar',
                                                       'stream']
    lo, hi = (int(re.search(r'#define %s (\d+)' % n, hdr).group(1)) for n in ('PCP_PFN_TRAIN_MIN_RAW', 'PCP_PFN_TRAIN_MAX_RAW'))
    assert (lo, hi) == (3, 26) == (tops.PFN_TRAIN_MIN_RAW, tops.PFN_TRAIN_MAX_RAW) == (dpv.TRAIN_MIN_RAW, dpv.TRAIN_MAX_RAW)
    assert 'pcp_pfn_train_features_w' in lib.SYMBOLS
    fn = lib.load().pcp_pfn_train_features_w                   # resolves in the built library
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(args) == 10
    assert [fn.argtypes[i] for i in (1, 2, 3, 4)] == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    assert len(lib.load().pcp_pfn_train_features.argtypes) == 9


def test_withmap_yaml_builds_a_trainable_vfe_on_the_layer_wise_inference_path():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    path = os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_withmap.yaml')
    cfg = cfg_from_yaml_file(path, EasyDict())
    vs = [p['VOXEL_SIZE'] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(cfg.DATA_CONFIG.POINT_FEATURE_ENCODING.used_feature_list))
    vfe = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).vfe
    assert vfe.num_raw_point_features == 10 and ds.point_feature_encoder.num_point_features == 12
    assert vfe.train_fused and not vfe.fused
    assert tuple(vfe.pfn_layers[0].linear.weight.shape) == (32, 16)
    assert 'layers' in vfe._build_packed()                     # eval keeps _forward_layers: per-layer packed weights, not w0 / w1


def test_train_mode_forward_refuses_a_cpu_tensor():
    """no CPU fall-back: a trainable width still says that the hot path needs device tensors, and leaves the module untouched"""
    from pcp_amd.lib import PcpError
    v = _vfe(10).train()
    before = {k: t.clone() for k, t in v.state_dict().items()}
    with pytest.raises(PcpError, match='no CPU fallback'):
        v({'points': torch.zeros(8, 13), 'batch_size': 2})
    assert all(torch.equal(before[k], t) for k, t in v.state_dict().items())


def test_g23_fixture_loads_and_describes_the_three_widths():
    assert os.path.getsize(os.path.join(GOLDEN, 'g23_vfe_train_widths.npz')) < MiB
    g = load_golden('g23_vfe_train_widths.npz')
    meta = g['meta']
    assert {t: (c['num_raw'], c['F']) for t, c in meta['cases'].items()} == {'w10': (10, 16), 'w7': (7, 13), 'w12': (12, 18)}
    assert meta['pc_range'] == [-12.8, -12.8, -8.0, 12.8, 12.8, 0.0] and meta['voxel_size'] == [0.2, 0.2, 8.0] and meta['grid_size'] == [128, 128, 1]
    for tag, c in meta['cases'].items():
        v = _vfe(c['num_raw'])
        assert v.train_fused and not v.fused
        assert {'vfe.' + k: list(t.shape) for k, t in v.state_dict().items()} == c['state_shapes'], tag
        assert c['relu_gap'] >= 1e-4 and c['top2_gap'] >= 1e-5 and c['bn_eps'] == 1e-3 and c['bn_momentum'] == 0.01
        pts = g[tag + '/points']
        assert pts.shape[1] == 1 + c['num_raw'] and set(np.unique(pts[:, 0])) == {0.0, 1.0}
        P = c['pillars']
        assert g[tag + '/voxel_coords'].shape == (P, 4) and g[tag + '/pillar_features'].shape == (P, 64)
        assert c['longest_pillars'][-6:] == [16, 17, 33, 40, 300, 1500]              # both sides of the 16 / 17 boundary and the long forms
        params = dict(v.named_parameters())
        assert c['param_names'] == list(params) and len(params) == 6
        for n, p in params.items():
            assert g['%s/g/%s' % (tag, n)].shape == tuple(p.shape) and np.isfinite(g['%s/g/%s' % (tag, n)]).all(), (tag, n)
            assert float(np.abs(g['%s/g/%s' % (tag, n)]).max()) > 0, (tag, n)
        for li in range(2):
            for k in ('running_mean', 'running_var'):
                assert g['%s/bn/pfn_layers.%d.norm.%s' % (tag, li, k)].shape == (32 * (li + 1),)
            assert int(g['%s/bn/pfn_layers.%d.norm.num_batches_tracked' % (tag, li)]) == 1
