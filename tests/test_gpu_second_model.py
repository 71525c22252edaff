"""VoxelResBackBone8x + HeightCompression against the float64 restatement of the whole stack, and the v2x_second_ego model end to end at a
mini range: build_network, model(batch), tools/test.py, the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
for p in (os.path.join(REPO, 'tests'), PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import spconv_refs as sr  # noqa: E402
from pcp_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

MINI_RANGE = [-6.4, -6.4, -8.0, 6.4, 6.4, 0.0]            # 128 x 128 x 40 voxels of (0.1, 0.1, 0.2)
YAML = 'cfgs/v2x_sim_models/v2x_second_ego.yaml'


def seeded_backbone():
    """the conditioned seeded case of tests/spconv_refs.py loaded into the modules"""
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.map_to_bev import HeightCompression
    from pcdet.models.backbones_3d import VoxelResBackBone8x
    D, H, W = sr.SECOND_GRID
    bb = VoxelResBackBone8x(EasyDict({'NAME': 'VoxelResBackBone8x'}), input_channels=11, grid_size=np.asarray([W, H, D]))
    st, feats, coords, want, pre = sr.second_backbone_case({k: tuple(v.shape) for k, v in bb.state_dict().items()})
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    hc = HeightCompression(EasyDict({'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256}))
    return bb.cuda().eval(), hc, feats, coords, want, pre


def test_backbone_and_height_compression_match_float64():
    """The input is conditioned (spconv_refs.second_backbone_case): no pre-ReLU value of the restatement lies within SECOND_MARGIN = 2e-4 of
    zero (smallest: 3.0e-4), which is asserted to be at least ten times the difference measured here.  Measured on the MI355X: max |spatial_features - float64| = 2.22e-6 on maps up to
    1.45 (2 544 voxels)."""
    bb, hc, feats, coords, want, pre = seeded_backbone()
    B = 2
    batch = {'voxel_features': torch.from_numpy(feats).cuda(), 'voxel_coords': torch.from_numpy(coords).cuda(), 'batch_size': B}
    with torch.no_grad():
        batch = hc(bb(batch))
    torch.cuda.synchronize()
    got = batch['spatial_features'].cpu().numpy()
    assert got.shape == want.shape == (B, 256, 6, 7) and batch['spatial_features_stride'] == 8
    assert batch['encoded_spconv_tensor'].spatial_shape == [2, 6, 7]
    assert [batch['multi_scale_3d_features'][k].spatial_shape for k in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4')] == \
        [[41, 48, 56], [21, 24, 28], [11, 12, 14], [5, 6, 7]]
    err = float(np.abs(got - want).max())
    near = min(float(np.abs(p).min()) for p in pre)
    print('SECOND backbone: max |spatial_features - float64| = %.3g, max |float64| = %.3g, %d voxels, smallest |pre-ReLU| = %.3g'
          % (err, float(np.abs(want).max()), len(coords), near))
    assert np.abs(want).max() > 0.1 and (want != 0).mean() > 0.05
    assert all(0.05 < float((p > 0).mean()) < 0.95 for p in pre)                         # every ReLU has rows on both of its sides
    assert err < 1e-3
    assert near >= sr.SECOND_MARGIN and near >= 10 * err                                 # no value of the restatement near a ReLU kink
    with torch.no_grad():
        again = hc(bb({'voxel_features': torch.from_numpy(feats).cuda(), 'voxel_coords': torch.from_numpy(coords).cuda(), 'batch_size': B}))
    assert torch.equal(again['spatial_features'], batch['spatial_features'])


def mini_model():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import SyntheticV2XDataset
    from pcdet.models import build_network
    cwd = os.getcwd()
    os.chdir(os.path.join(PKG, 'tools'))
    try:
        cfg = cfg_from_yaml_file(YAML, EasyDict())
    finally:
        os.chdir(cwd)
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=4000, NUM_FRAMES=3, DISTRIBUTION='uniform')
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval(), ds


def _preds(model, ds, idx):
    from pcdet.models import load_data_to_gpu
    batch = ds.collate_batch([ds[i] for i in idx])
    load_data_to_gpu(batch)
    with torch.no_grad():
        pred, _ = model(batch)
    torch.cuda.synchronize()
    return [(p['pred_boxes'].cpu().numpy(), p['pred_scores'].cpu().numpy(), p['pred_labels'].cpu().numpy()) for p in pred], batch


def test_model_builds_runs_repeats_and_is_batch_invariant():
    model, ds = mini_model()
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelResBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                              'CenterHead']
    assert list(ds.grid_size) == [128, 128, 40]
    full, batch = _preds(model, ds, [0, 1, 2])
    assert batch['voxel_coords'].shape[0] > 100 and batch['spatial_features'].shape == (3, 256, 16, 16)
    assert batch['voxel_features'].shape[1] == 11
    for boxes, scores, labels in full:
        assert boxes.ndim == 2 and boxes.shape[1] == 7 and np.isfinite(boxes).all() and np.isfinite(scores).all()
    again, _ = _preds(model, ds, [0, 1, 2])
    for a, b in zip(full, again):
        for u, v in zip(a, b):
            assert u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8))
    for i in range(3):
        alone, _ = _preds(model, ds, [i])
        for u, v in zip(alone[0], full[i]):
            assert u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), i


def test_refusals():
    from pcdet.models.graphed import GraphedDetector
    from pcdet.models.pipelined import PipelinedDetector
    model, ds = mini_model()
    with pytest.raises(NotImplementedError, match='inference only'):
        model.train()
    model.eval()
    assert not PipelinedDetector.supports(model)
    with pytest.raises(NotImplementedError, match='VoxelResBackBone8x'):
        PipelinedDetector(model)
    with pytest.raises(NotImplementedError, match='VoxelResBackBone8x'):
        GraphedDetector(model, torch.zeros((4, 14), device='cuda'), 1, [{}])
    # nz > 64: the VFE refuses a grid of more than 64 cells along z, with the number
    model.vfe.grid_size = [128, 128, 80]
    model.vfe.voxel_size = [0.1, 0.1, 0.1]
    with pytest.raises(ValueError, match='80'):
        _preds(model, ds, [0])


@pytest.mark.parametrize('extra', [[], ['--device_eval'], ['--fast']])
def test_tools_test_py_runs_the_second_yaml(extra):
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', YAML, '--batch_size', '2'] + extra + \
          ['--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE), 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '3000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '3', 'DATA_CONFIG.SYNTHETIC.EVAL_GT', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    out = r.stdout + r.stderr
    assert ('mean_ap' in out) if extra == ['--device_eval'] else ('over 3 frames' in out), out[-1500:]
