"""pcp_pillar_vfe and the PillarVFE module on the GPU against tests/golden/g29_pillar_vfe.npz (the reference's own PillarVFE and
PointPillarScatter on the CPU) and the float64 restatement; the classic PointPillar YAML through model(batch) and tools/test.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
for p in (os.path.join(REPO, 'tests'), PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import hard_voxel_refs as hv  # noqa: E402
from pcp_amd import ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-3                    # the project's standing parity bar
CASES = ['norm4', 'nonorm5', 'dist4', 'noabs5']


@pytest.fixture(scope='module')
def golden():
    return load_golden('g29_pillar_vfe.npz')


def build_vfe(g, tag, with_voxeliser=False):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d import vfe
    case, meta = g['meta']['cases'][tag], g['meta']
    mc = EasyDict(NAME='PillarVFE', WITH_DISTANCE=case['with_distance'], USE_ABSLOTE_XYZ=case['use_absolute_xyz'], USE_NORM=case['use_norm'],
                  NUM_FILTERS=[case['width']])
    kw = {}
    if with_voxeliser:
        kw['hard_voxel'] = {'MAX_POINTS_PER_VOXEL': meta['max_points_per_voxel'],
                            'MAX_NUMBER_OF_VOXELS': {'train': meta['max_number_of_voxels'], 'test': meta['max_number_of_voxels']}}
    m = vfe.__all__['PillarVFE'](model_cfg=mc, num_point_features=case['num_raw'], voxel_size=meta['voxel_size'],
                                 point_cloud_range=np.asarray(meta['pc_range'], np.float32), grid_size=meta['grid_size'], **kw)
    m.load_state_dict({k: torch.from_numpy(g['%s/state/%s' % (tag, k)]) for k in case['state_keys']})
    return m.cuda().eval()


def voxel_keys(g, tag):
    return {'voxels': torch.from_numpy(g[tag + '/voxels']).cuda(), 'voxel_num_points': torch.from_numpy(g[tag + '/voxel_num_points']).cuda(),
            'voxel_coords': torch.from_numpy(g[tag + '/voxel_coords']).cuda(), 'batch_size': g['meta']['batch_size']}


def folded64(g, tag):
    case = g['meta']['cases'][tag]
    s = lambda k: g['%s/state/pfn_layers.0.%s' % (tag, k)]                       # noqa: E731
    if case['use_norm']:
        return hv.fold_bn(s('linear.weight'), s('norm.weight'), s('norm.bias'), s('norm.running_mean'), s('norm.running_var'))
    return s('linear.weight').astype(np.float64), s('linear.bias').astype(np.float64)


@pytest.mark.parametrize('tag', CASES)
def test_pillar_features_match_the_reference(golden, tag):
    g, meta, case = golden, golden['meta'], golden['meta']['cases'][tag]
    m = build_vfe(g, tag)
    with torch.no_grad():
        bd = m(voxel_keys(g, tag))
    got = bd['pillar_features'].cpu().numpy()
    want = g[tag + '/pillar_features']
    assert got.shape == want.shape == (case['pillars'], case['width'])
    err = float(np.abs(got - want).max())
    w64, b64 = folded64(g, tag)
    r = np.asarray(meta['pc_range'], np.float32)
    offset = [meta['voxel_size'][j] / 2 + r[j] for j in range(3)]
    ref64 = hv.pillar_vfe_ref(g[tag + '/voxels'], g[tag + '/voxel_num_points'], g[tag + '/voxel_coords'], meta['voxel_size'], offset, w64, b64,
                              case['use_absolute_xyz'], case['with_distance'])
    err64 = float(np.abs(got - ref64).max())
    print('%s: max |pillar_features - fixture| = %.3g, - float64 restatement = %.3g' % (tag, err, err64))
    assert err < TOL, err
    assert err64 < TOL, err64


@pytest.mark.parametrize('tag', ['norm4', 'nonorm5', 'dist4'])
def test_padded_slots_take_part_in_the_max(golden, tag):
    g, case = golden, golden['meta']['cases'][tag]
    m = build_vfe(g, tag)
    with torch.no_grad():
        pf = m(voxel_keys(g, tag))['pillar_features'].cpu().numpy()
    ch, bias = case['pad_channel'], np.float32(case['pad_bias'])
    num = g[tag + '/voxel_num_points']
    T = g['meta']['max_points_per_voxel']
    assert num[case['short_pillar']] < T and num[case['full_pillar']] == T
    assert np.all(pf[num < T, ch] == bias)                  # every pillar with a zero row: ReLU(bias) exactly
    for i in case['full_pillars']:                          # a full pillar has no zero row: its true maximum, below ReLU(bias)
        assert pf[i, ch] < bias
        assert abs(pf[i, ch] - g[tag + '/pillar_features'][i, ch]) < TOL


def test_module_spatial_features_and_points_path(golden):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.map_to_bev import PointPillarScatter
    g, meta, tag = golden, golden['meta'], 'norm4'
    m = build_vfe(g, tag, with_voxeliser=True)
    scatter = PointPillarScatter(model_cfg=EasyDict(NAME='PointPillarScatter', NUM_BEV_FEATURES=64), grid_size=meta['grid_size'])
    with torch.no_grad():
        fed = scatter(m(voxel_keys(g, tag)))
        from_points = {'points': torch.from_numpy(g[tag + '/points']).cuda(), 'batch_size': meta['batch_size']}
        own = scatter(m(from_points))
    want = g[tag + '/spatial_features']
    got = fed['spatial_features'].cpu().numpy()
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) < TOL
    # the module fed `points` only: the op's voxel tensors, written back under the reference's keys, and the same features
    grid = ops.make_grid(meta['pc_range'], meta['voxel_size'], meta['grid_size'], meta['batch_size'])
    res = ops.hard_voxelize(from_points['points'], grid, meta['pc_range'][5], meta['max_points_per_voxel'], meta['max_number_of_voxels'])
    for key, t in (('voxels', res.voxels), ('voxel_coords', res.voxel_coords), ('voxel_num_points', res.voxel_num_points)):
        assert torch.equal(own[key], t), key
        assert np.array_equal(own[key].cpu().numpy(), g['%s/%s' % (tag, key)]), key          # = the restatement's, stored with the fixture
    assert torch.equal(own['pillar_features'], fed['pillar_features'])
    assert torch.equal(own['spatial_features'], fed['spatial_features'])


def test_module_refuses_training():
    g = load_golden('g29_pillar_vfe.npz')
    m = build_vfe(g, 'norm4')
    with pytest.raises(NotImplementedError, match='inference only'):
        m.train()


def small_model():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import SyntheticV2XDataset
    from pcdet.models import build_network
    cwd = os.getcwd()
    os.chdir(os.path.join(PKG, 'tools'))
    try:
        cfg = cfg_from_yaml_file('cfgs/v2x_sim_models/v2x_pointpillar_anchor_hardvoxel.yaml', EasyDict())
    finally:
        os.chdir(cwd)
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = [-12.8, -12.8, -8.0, 12.8, 12.8, 0.0]            # 128 x 128 cells
    # the synthetic car cloud spreads over +-52 m: about 1 200 of the 20 000 rows of a frame fall inside the small range
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=20000, NUM_FRAMES=2, DISTRIBUTION='uniform')
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval(), ds


def test_model_forward_is_finite_and_repeats():
    from pcdet.models import load_data_to_gpu
    model, ds = small_model()
    outs = []
    for _ in range(2):
        batch = ds.collate_batch([ds[0], ds[1]])
        load_data_to_gpu(batch)
        with torch.no_grad():
            pred, _ = model(batch)
        torch.cuda.synchronize()
        assert batch['voxels'].shape[1:] == (32, 7) and batch['voxel_coords'].shape[0] == batch['voxels'].shape[0] > 0
        outs.append([(p['pred_boxes'].cpu().numpy(), p['pred_scores'].cpu().numpy(), p['pred_labels'].cpu().numpy()) for p in pred])
    assert len(outs[0]) == 2
    for a, b in zip(outs[0], outs[1]):
        for x, y in zip(a, b):
            assert np.isfinite(x).all()
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_tools_test_py_runs_the_hardvoxel_yaml():
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', 'cfgs/v2x_sim_models/v2x_pointpillar_anchor_hardvoxel.yaml', '--batch_size', '2', '--set',
           'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '4000', 'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '4']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    assert 'detections over 4 frames' in r.stdout + r.stderr
