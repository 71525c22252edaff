"""Training v2x_second_ego on HIP: VoxelBackboneTrain + HeightCompression forward and backward against the float64 autograd restatement of
tests/spconv_train_refs.py under batch-statistics BatchNorm, one training iteration of the mini model built with the HIP_TRAIN switch, and
tools/train.py with and without it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
for p in (os.path.join(REPO, 'tests'), PKG, os.path.join(PKG, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import spconv_train_refs as tr  # noqa: E402
from pcp_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

MINI_RANGE = [-6.4, -6.4, -8.0, 6.4, 6.4, 0.0]            # 128 x 128 x 40 voxels of (0.1, 0.1, 0.2)
YAML = 'cfgs/v2x_sim_models/v2x_second_ego.yaml'
PARITY_BAR = 1e-3
# max |gpu - f64| / max |f64| per tensor, measured once on the MI355X (tests/golden/second_train_measured.json); the test allows ten times
# that, capped by the project's 1e-3 parity bar
MEASURED = os.path.join(REPO, 'tests', 'golden', 'second_train_measured.json')


def backbone_modules():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.map_to_bev import HeightCompression
    from pcdet.models.backbones_3d import VoxelResBackBone8x
    D, H, W = tr.TRAIN_GRID
    bb = VoxelResBackBone8x(EasyDict({'NAME': 'VoxelResBackBone8x', 'HIP_TRAIN': True}), input_channels=11, grid_size=np.asarray([W, H, D]))
    hc = HeightCompression(EasyDict({'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 128}))
    return bb, hc


def backbone_case():
    bb, hc = backbone_modules()
    st, feats, coords, dcanvas, want, pre = tr.second_train_case({k: tuple(v.shape) for k, v in bb.state_dict().items()})
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return bb.cuda().train(), hc.train(), st, feats, coords, dcanvas, want, pre


def run_backbone_case():
    """-> (relative differences {tensor name: max |gpu - f64| / max |f64|}, absolute bias differences {name: (|diff|, max |weight.grad|)},
    forward difference, smallest |pre-ReLU| of the restatement, the gradient tensors)"""
    from pcp_amd import ops
    from pcp_amd import train_layers as tl
    from pcp_amd.train_layers import Act
    bb, hc, st, feats, coords, dcanvas, want, pre = backbone_case()
    batch = {'voxel_features': torch.from_numpy(feats).cuda(), 'voxel_coords': torch.from_numpy(coords).cuda(), 'batch_size': 2}
    batch = hc(bb(batch))
    tape = batch['_pcp_tape']
    assert [n for n, _ in tape] == ['backbone_3d', 'map_to_bev']
    g = Act(ops.as_nhwc(torch.from_numpy(dcanvas).cuda()))
    for _name, fn in reversed(tape):
        g = fn(g)
    assert g is None
    tl.flush_batches_tracked()
    torch.cuda.synchronize()
    rel = lambda got, ref: float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
    sf = batch['spatial_features'].cpu().numpy()
    assert sf.shape == want['spatial_features'].shape
    out = {'spatial_features': rel(sf, want['spatial_features'])}
    fwd = float(np.abs(sf - want['spatial_features']).max())
    sd = bb.state_dict()
    for k, v in want['running'].items():
        out[k] = rel(sd[k].cpu().numpy(), v)
    for k, v in sd.items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1, k
    bias_abs, grads = {}, {}
    for name, p in bb.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        got, ref = p.grad.cpu().numpy(), want['grads'][name]
        grads[name] = got
        if name.endswith('conv1.bias') or name.endswith('conv2.bias'):
            wref = want['grads'][name[:-4] + 'weight']
            bias_abs[name] = (float(np.abs(got - ref).max()), float(np.abs(wref).max()))
        else:
            out[name] = rel(got, ref)
    near = min(float(np.abs(p).min()) for p in pre)
    return out, bias_abs, fwd, near, grads


def test_backbone_training_forward_and_backward_match_float64():
    """Measured on the MI355X (one run): see tests/golden/second_train_measured.json, the README section quotes the largest values."""
    out, bias_abs, fwd, near, _ = run_backbone_case()
    measured = json.load(open(MEASURED))
    worst = max(out.values())
    print('SECOND training backbone: forward max |diff| %.3g, smallest |pre-ReLU| %.3g, largest relative difference %.3g (%s)'
          % (fwd, near, worst, max(out, key=out.get)))
    for k, v in sorted(out.items()):
        print('  %-40s %.3g' % (k, v))
    assert near >= tr.TRAIN_MARGIN and near >= 10 * fwd                                   # no value of the restatement near a ReLU kink
    assert set(out) == set(measured)
    bad = {k: (v, measured[k]) for k, v in out.items() if not v <= min(PARITY_BAR, 10 * measured[k])}
    assert not bad, bad
    badb = {k: v for k, v in bias_abs.items() if not v[0] <= 1e-3 * v[1]}
    assert not badb, badb


def mini_model(switch=True):
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
    if switch:
        cfg.MODEL.VFE.HIP_TRAIN = True
        cfg.MODEL.BACKBONE_3D.HIP_TRAIN = True
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda(), ds, cfg


def _batch(ds, idx):
    from pcdet.models import load_data_to_gpu
    batch = ds.collate_batch([ds[i] for i in idx])
    load_data_to_gpu(batch)
    return batch


def _first_step():
    from train_utils.optimization import build_optimizer, build_scheduler
    model, ds, cfg = mini_model()
    opt = build_optimizer(model, cfg.OPTIMIZATION)
    sched, _ = build_scheduler(opt, 5, cfg.OPTIMIZATION.NUM_EPOCHS, -1, cfg.OPTIMIZATION)
    sched.step(0)
    model.train()
    opt.zero_grad()
    ret, _tb, _disp = model(_batch(ds, [0, 1]))
    model.update_global_step()
    ret['loss'].backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return float(ret['loss'].detach()), grads, (model, opt, ds)


@pytest.fixture(scope='module')
def first_step():
    return _first_step()


def test_one_iteration_gives_every_parameter_a_finite_gradient(first_step):
    loss, grads, (model, _opt, _ds) = first_step
    assert np.isfinite(loss)
    names = [n for n in grads if n.split('.')[0] in ('backbone_3d', 'backbone_2d', 'dense_head')]
    assert len([n for n in names if n.startswith('backbone_3d.')]) == 21 + 8 * 2 + 21 * 2      # 21 conv weights, 16 block biases, 21 BatchNorms
    for n in names:
        assert grads[n] is not None and torch.isfinite(grads[n]).all(), n
    assert all(float(grads[n].abs().max()) > 0 for n in names if n.endswith('.weight'))


def test_the_iteration_repeats_bit_for_bit(first_step):
    la, ga, _ = first_step
    lb, gb, _ = _first_step()
    assert la == lb and set(ga) == set(gb)
    assert not [n for n in ga if ga[n] is not None and not torch.equal(ga[n], gb[n])]


def test_eval_after_an_optimizer_step_uses_the_stepped_weights(first_step):
    _loss, _grads, (model, opt, ds) = first_step
    fresh, _, _ = mini_model()
    fresh.eval()
    with torch.no_grad():
        before, _ = fresh(_batch(ds, [0, 1]))
    opt.step()
    model.eval()
    with torch.no_grad():
        after, _ = model(_batch(ds, [0, 1]))
    torch.cuda.synchronize()
    assert all(np.isfinite(p['pred_scores'].cpu().numpy()).all() for p in after)
    same = all(a['pred_boxes'].shape == b['pred_boxes'].shape and torch.equal(a['pred_boxes'], b['pred_boxes'])
               and torch.equal(a['pred_scores'], b['pred_scores']) for a, b in zip(after, before))
    assert not same                                                                       # the packed caches were dropped


def test_bf16_loop_iteration_is_finite(monkeypatch):
    """the sparse stage stays fp32; the canvas goes to BackboneTrain as bf16 and the canvas gradient comes back as float32"""
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    loss, grads, _ = _first_step()
    assert np.isfinite(loss)
    assert all(g is not None and torch.isfinite(g).all() for n, g in grads.items() if n.split('.')[0] in ('backbone_3d', 'backbone_2d', 'dense_head'))


def test_an_empty_batch_passes_through():
    from pcp_amd.train_layers import Act
    bb, hc = backbone_modules()
    bb, hc = bb.cuda().train(), hc.train()
    batch = {'voxel_features': torch.zeros((0, 11), device='cuda'), 'voxel_coords': torch.zeros((0, 4), dtype=torch.int32, device='cuda'),
             'batch_size': 2}
    batch = hc(bb(batch))
    assert tuple(batch['spatial_features'].shape) == (2, 128, 4, 4) and float(batch['spatial_features'].abs().max()) == 0.0
    g = Act(torch.ones((2, 4, 4, 128), device='cuda'))
    for _name, fn in reversed(batch['_pcp_tape']):
        g = fn(g)
    for name, p in bb.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, name
    assert all(int(v) == 0 for k, v in bb.state_dict().items() if k.endswith('num_batches_tracked'))


def test_without_the_switch_train_is_refused():
    model, _ds, _cfg = mini_model(switch=False)
    with pytest.raises(NotImplementedError, match='inference only'):
        model.train()
    from pcp_amd import spconv
    conv = spconv.SubMConv3d(16, 16, 3).cuda().train()
    x = spconv.SparseConvTensor(torch.zeros((1, 16), device='cuda'), torch.zeros((1, 4), dtype=torch.int32, device='cuda'), [3, 3, 3], 1)
    with pytest.raises(NotImplementedError, match='inference only'):
        conv(x)
    with pytest.raises(NotImplementedError, match='inference only'):
        spconv.SparseSequential(conv).train()(x)


def _train_py(tmp_path, extra):
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'train.py', '--cfg_file', YAML, '--batch_size', '2', '--epochs', '1', '--output_dir', str(tmp_path), '--set',
           'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE), 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '3000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '4'] + extra
    return subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=600)


def test_train_py_runs_one_epoch_with_the_switch(tmp_path):
    r = _train_py(tmp_path, ['MODEL.VFE.HIP_TRAIN', 'True', 'MODEL.BACKBONE_3D.HIP_TRAIN', 'True'])
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    ck = torch.load(os.path.join(str(tmp_path), 'ckpt', 'checkpoint_epoch_1.pth'), map_location='cpu', weights_only=False)
    assert ck['it'] == 2 and all(torch.isfinite(v).all() for v in ck['model_state'].values() if v.dtype.is_floating_point)


def test_train_py_without_the_switch_fails_with_the_message(tmp_path):
    r = _train_py(tmp_path, [])
    assert r.returncode != 0 and 'inference only' in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2000:]
