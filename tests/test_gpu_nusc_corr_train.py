"""Training pointpillar_jr_corr_withmap on the GPU: the box filter at any row width (pcp_filter_gt_boxes_w), the whole model on the 60 x 60
mini grid of g24_corr_mini with the synthetic loader's HD-map training batch (VFE -> scatter -> SCBackboneTrain -> HunterTrain -> HeadTrain),
pointpillar_jr_withmap on the same batch, and tools/train.py on the corrector YAML."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
CFGS = os.path.join(PKG, 'tools', 'cfgs', 'nuscenes_models')
MINI_RANGE = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]
CORR_TERMS = ('l_points_cls', 'l_points_embed', 'l_fg_offset', 'l_locals_transl', 'l_locals_rot', 'l_recon', 'l_dtl_locals_feat')


# ---- box filter -----------------------------------------------------------------------------------------------------------------------

def _filter_numpy(gt, rng):
    """remove_gt_boxes_outside_range (hunter_toolbox.py:161-184) for rows of any width, M kept: ordered compaction, zero padding"""
    out = np.zeros_like(gt)
    for b in range(gt.shape[0]):
        c = gt[b, :, :3]
        keep = np.all((c >= np.float32(rng[:3])) & (c < np.float32(rng[3:])), axis=1)
        out[b, :int(keep.sum())] = gt[b, keep]
    return out


def _boxes(width, seed=11):
    """(4, 7, width): frame 0 has one row outside on x and one on y, frame 1 every row outside, frame 2 none, frame 3 padding rows between"""
    rs = np.random.RandomState(seed)
    gt = rs.uniform(-4.0, 4.0, size=(4, 7, width)).astype(np.float32)
    gt[..., 2] = rs.uniform(-4.0, 2.0, size=(4, 7))
    gt[..., width - 1] = rs.randint(1, 11, size=(4, 7))
    gt[0, 2, 0] = 6.5
    gt[0, 5, 1] = -6.25
    gt[1, :, 0] = 7.0 + np.arange(7)
    gt[3, 1] = 0.0                                  # a padding row has its centre at the origin: inside, kept in place
    gt[3, 4, 2] = 3.0                               # z on the upper bound is outside (half-open interval)
    return gt


def test_box_filter_width_10_matches_the_numpy_restatement():
    from pcp_amd import train_ops as tops
    gt = _boxes(10)
    want = _filter_numpy(gt, MINI_RANGE)
    assert (want[0, 5:] == 0).all() and want[0, 4].any() and not want[1].any() and np.array_equal(want[2], gt[2])
    got = tops.filter_gt_boxes(torch.from_numpy(gt).to(DEV), MINI_RANGE).cpu().numpy()
    assert got.shape == (4, 7, 10) and np.array_equal(got, want)
    for width in (9, 16):                           # every width up to the limit, odd ones included
        g = _boxes(width, seed=width)
        assert np.array_equal(tops.filter_gt_boxes(torch.from_numpy(g).to(DEV), MINI_RANGE).cpu().numpy(), _filter_numpy(g, MINI_RANGE))
    big = np.tile(_boxes(10), (1, 43, 1))[:, :300]  # more rows than one pass of the workgroup
    assert np.array_equal(tops.filter_gt_boxes(torch.from_numpy(big).to(DEV), MINI_RANGE).cpu().numpy(), _filter_numpy(big, MINI_RANGE))


def test_box_filter_width_8_is_bit_equal_to_the_fixed_width_entry():
    from pcp_amd import lib
    from pcp_amd import train_ops as tops
    gt = torch.from_numpy(_boxes(8)).to(DEV)
    old = torch.full_like(gt, 7.0)
    rng = (ctypes.c_float * 6)(*MINI_RANGE)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.load().pcp_filter_gt_boxes(ctypes.c_void_p(gt.data_ptr()), 4, 7, rng, ctypes.c_void_p(old.data_ptr()), st)
    assert rc == 0
    new = tops.filter_gt_boxes(gt, MINI_RANGE)
    torch.cuda.synchronize()
    assert torch.equal(old, new) and np.array_equal(new.cpu().numpy(), _filter_numpy(gt.cpu().numpy(), MINI_RANGE))
    bad = torch.zeros((1, 3, 17), device=DEV)
    out = torch.zeros_like(bad)
    rc = lib.load().pcp_filter_gt_boxes_w(ctypes.c_void_p(bad.data_ptr()), 1, 3, 17, rng, ctypes.c_void_p(out.data_ptr()), st)
    assert rc != 0                                   # the C entry refuses it too, before a launch


# ---- HunterTrain against the reference's own HunterJr in train() mode (g25) ---------------------------------------------------------------

def _sample(t, n):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)][:n].cpu().numpy()


def test_hunter_train_matches_the_reference_module():
    """tests/golden/g25_corr_train.npz: hidden width 64, NUM_SWEEPS 10, 13-column rows, 10-column gt_boxes, the upstream gradient fed to
    backward.  Meta, class targets and gt_boxes_after exact; predictions and points to 1e-3, the map probe to 2e-4, the seven terms to 1e-4
    relative, gradients under the rule of g12 (inside the noise band, global relative L2 <= 2e-2), running statistics to 1e-5."""
    from pcdet.config import EasyDict
    from pcdet.models.bev_layers.hunter_jr import HunterJr
    from pcp_amd.train_layers import Act
    g = load_golden('g25_corr_train.npz')
    meta = g['meta']
    state = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    for k, v in meta['state_overrides'].items():
        state[k] = np.asarray(v, dtype=np.float32)
    corr = HunterJr(EasyDict(meta['corrector']), meta['num_bev_features'], meta['voxel_size'], meta['pc_range'])
    corr.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    corr = corr.to(DEV).train()
    mp, up = meta['map'], meta['upstream']
    n = int(np.prod(mp['shape']))
    x = synth.uniform(mp['seed'], mp['stream'], n, mp['lo'], mp['hi']).reshape(mp['shape'])
    dfused = ((synth.uniform01(up['seed'], up['stream'], n).astype(np.float64) - 0.5) * 2 * up['scale']).astype(np.float32).reshape(mp['shape'])
    assert g['gt_boxes'].shape == (2, 7, 10) and g['points'].shape[1] == 13 and int(corr.num_sweeps) == 10
    bd = {'points': torch.from_numpy(g['points'].copy()).to(DEV), 'spatial_features_2d': torch.from_numpy(x).to(DEV), 'batch_size': 2,
          'metadata': [{}, {}], 'gt_boxes': torch.from_numpy(g['gt_boxes']).to(DEV), 'instances_tf': torch.from_numpy(g['instances_tf']).to(DEV)}
    bd = corr(bd)
    tb = {}
    loss, tb = corr.get_training_loss(tb)
    dx = corr._pcp_train.backward(Act(torch.from_numpy(dfused).to(DEV).permute(0, 2, 3, 1).contiguous()))
    torch.cuda.synchronize()
    fr = corr.forward_return_dict
    m = fr['meta']
    assert np.array_equal(m.fg_local[:m.n_fg].cpu().numpy(), g['meta/locals2fg'])
    assert np.array_equal(m.local_key[:m.n_local].cpu().numpy(), g['meta/locals_bis'])
    assert np.array_equal(m.inst_key[:m.n_inst].cpu().numpy(), g['meta/instance_bi'])
    assert np.array_equal(fr['points_cls_target'].cpu().numpy(), g['tgt/points_cls'])
    lo = corr._pcp_train.s['loss_out']
    np.testing.assert_allclose(lo['tgt_embedding'].cpu().numpy(), g['tgt/fg_embedding'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(lo['tgt_offset'].cpu().numpy(), g['tgt/fg_offset'], rtol=0, atol=1e-5)
    for k in ('points_cls_logit', 'points_flow3d', 'points_embedding', 'locals_tf'):
        np.testing.assert_allclose(fr['prediction'][k].detach().cpu().numpy(), g['pred/' + k], rtol=0, atol=1e-3, err_msg=k)
    np.testing.assert_allclose(bd['points'].cpu().numpy(), g['points_after'], rtol=0, atol=1e-3)
    ga, gb = g['gt_boxes_after'], bd['gt_boxes'].cpu().numpy()
    assert ga.shape[2] == gb.shape[2] == 10 and np.array_equal(gb[:, :ga.shape[1]], ga) and not gb[:, ga.shape[1]:].any()
    np.testing.assert_allclose(bd['spatial_features_2d'].detach().cpu().numpy()[:, ::4], g['map_probe'], rtol=0, atol=2e-4)
    names = ('l_points_cls', 'l_points_embed', 'l_fg_offset', 'l_locals_transl', 'l_locals_rot', 'l_recon', 'l_dtl_locals_feat')
    for k, want in zip(names, g['losses'][:7]):
        print('%-18s %.7f  reference %.7f' % (k, tb[k], want))
        assert abs(tb[k] - want) <= 1e-4 * abs(want) + 1e-9, (k, tb[k], want)
    assert abs(float(loss) - g['losses'][7]) <= 1e-4 * abs(g['losses'][7])
    # gradients: parameters (strided samples) and the whole input map
    params = dict(corr.named_parameters())
    trainable = [str(k) for k in meta['trainable']]
    assert set(trainable) == set(params)
    refs = {k: g['g/' + k] for k in trainable}
    mine = {k: _sample(params[k].grad, meta['samples']) for k in trainable}
    refs['input map'] = g['dinput']
    mine['input map'] = dx.t[..., dx.off:dx.off + dx.c].float().permute(0, 3, 1, 2).cpu().numpy()
    gmax = max(float(np.abs(v).max()) for v in refs.values())
    num = den = 0.0
    for k, ref in refs.items():
        scale = max(float(np.abs(ref).max()), 1e-4 * gmax)
        assert np.abs(mine[k] - ref).max() <= 1e-1 * scale, (k, float(np.abs(mine[k] - ref).max()), scale)
        num += float(((mine[k].astype(np.float64) - ref) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
    print('global relative L2 of the gradients: %.3g' % (num / den) ** 0.5)
    assert num <= (2e-2 ** 2) * den, (num / den) ** 0.5
    sd = corr.state_dict()
    for k in [k for k in sd if k.endswith('running_mean') or k.endswith('running_var')]:
        np.testing.assert_allclose(sd[k].cpu().numpy(), g['bn/' + k], rtol=1e-5, atol=1e-5, err_msg=k)


# ---- whole model, mini geometry ----------------------------------------------------------------------------------------------------

def _loader_batch(yaml_name, frames=2, points_per_frame=600):
    """the synthetic loader's training batch of an HD-map YAML at the mini range (about 2 000 rows for two frames)"""
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    cfg = cfg_from_yaml_file(os.path.join(CFGS, yaml_name), EasyDict())
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_FRAME=points_per_frame, NUM_FRAMES=frames, DISTRIBUTION='uniform', XY_HALF=6.5)
    ds, _loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, frames, False, training=True)
    return ds.collate_batch([ds[i] for i in range(frames)]), cfg


@pytest.fixture(scope='module')
def mini():
    g = load_golden('g24_corr_mini.npz')
    meta = dict(g['meta']['cases']['corr'])
    assert [float(v) for v in meta['pc_range']] == MINI_RANGE
    batch, cfg = _loader_batch('pointpillar_jr_corr_withmap.yaml')
    meta['optimization'] = cfg.OPTIMIZATION
    meta['total_it_each_epoch'] = 5
    assert batch['points'].shape[1] == 13 and 1500 <= batch['points'].shape[0] <= 2500 and batch['gt_boxes'].shape[2] == 10
    return dict(meta=meta, batch=batch)


def _model_and_optimizer(meta):
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    from train_utils.optimization import build_optimizer, build_scheduler
    from pcdet.config import EasyDict
    from pcdet.models import build_network_from_meta
    model = build_network_from_meta(meta)
    st = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    for k, v in meta.get('state_overrides', {}).items():
        st[k] = np.asarray(v, dtype=np.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(DEV)
    ocfg = EasyDict(meta['optimization'])
    assert ocfg.OPTIMIZER == 'adam_onecycle'
    opt = build_optimizer(model, ocfg)
    sched, _ = build_scheduler(opt, meta['total_it_each_epoch'], ocfg.NUM_EPOCHS, -1, ocfg)
    return model, opt, sched, ocfg


def _device_batch(batch, train=True):
    out = {'points': torch.from_numpy(batch['points'].copy()).to(DEV), 'batch_size': batch['batch_size'], 'metadata': batch['metadata']}
    if train:
        out['gt_boxes'] = torch.from_numpy(batch['gt_boxes']).to(DEV)
        out['instances_tf'] = torch.from_numpy(batch['instances_tf']).to(DEV)
    return out


def _train_iterations(g, n_it):
    """n_it iterations of the reference's loop (train_utils.py:49-58); the loss, tb_dict and gradients of each; the model after the LAST
    optimizer step"""
    model, opt, sched, ocfg = _model_and_optimizer(g['meta'])
    its = []
    for it in range(n_it):
        sched.step(it)
        model.train()
        opt.zero_grad()
        ret, tb, _disp = model(_device_batch(g['batch']))
        model.update_global_step()
        ret['loss'].backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        its.append((float(ret['loss'].detach()), dict(tb), grads))
        opt.clip_grad_norm(ocfg.GRAD_NORM_CLIP)
        opt.step()
    return its, model


@pytest.fixture(scope='module')
def fp32_run(mini):
    return _train_iterations(mini, 2)


def test_corrector_model_trains_two_iterations(mini, fp32_run):
    its, model = fp32_run
    want = set(n for n, p in model.named_parameters() if p.requires_grad)
    assert any(n.startswith('corrector.object_head.') for n in want) and any(n.startswith('backbone_2d.') for n in want)
    for loss, tb, grads in its:
        assert np.isfinite(loss) and loss > 0
        keys = CORR_TERMS + ('loss_corrector', 'loss_rpn', 'rpn_loss', 'loss_total') + tuple('%s_loss_head_%d' % (k, h) for h in range(6)
                                                                                              for k in ('hm', 'loc'))
        assert not [k for k in keys if k not in tb or not np.isfinite(tb[k])], tb
        assert abs(sum(tb[k] for k in CORR_TERMS) - tb['loss_corrector']) <= 1e-5 * abs(tb['loss_corrector'])
        assert abs(tb['loss_rpn'] + tb['loss_corrector'] - loss) <= 1e-5 * abs(loss)
        assert all(tb[k] > 0 for k in CORR_TERMS), tb            # foreground, locals and moving instances are all present in the loader batch
        assert set(grads) == want
        bad = [n for n, v in grads.items() if not torch.isfinite(v).all()]
        assert not bad, bad
        for prefix in ('vfe.', 'backbone_2d.', 'corrector.conv_input.', 'corrector.point_head.', 'corrector.object_head.',
                       'corrector.conv_weightor.', 'dense_head.'):
            assert any(float(v.abs().max()) > 0 for n, v in grads.items() if n.startswith(prefix)), prefix
    assert its[0][0] != its[1][0]


def test_embedding_target_reads_gt_boxes_at_their_row_width(mini):
    """the loss kernel reads the box centre at the run-time row stride: tgt_embedding and l_points_embed of one forward on the loader's
    10-column boxes against a numpy restatement (hunter_jr.py:222-225, 420-421).  Instances 1..11 of both frames carry foreground, so a read
    at stride 8 lands in other rows.  gt_boxes after the forward is the numpy filter of the input, all 10 columns."""
    model, _opt, _sched, _ocfg = _model_and_optimizer(mini['meta'])
    model.train()
    bd = _device_batch(mini['batch'])
    ret, tb, _disp = model(bd)
    pts, gt = mini['batch']['points'], mini['batch']['gt_boxes']
    fg = np.nonzero(pts[:, -1] > -1)[0]
    frame, inst = pts[fg, 0].astype(int), pts[fg, -1].astype(int)
    assert inst.max() >= 8 and set(frame) == {0, 1} and gt.shape[2] == 10
    want = gt[frame, inst, :2] - pts[fg, 1:3]
    st = model.corrector._pcp_train.s
    assert np.array_equal(st['meta'].fg_idx[:st['meta'].n_fg].cpu().numpy(), fg)
    got = st['loss_out']['tgt_embedding'].cpu().numpy()
    assert np.array_equal(got, want)                                   # one float32 subtraction per value
    wrong = gt.reshape(-1)[((frame * gt.shape[1] + inst) * 8)[:, None] + np.arange(2)] - pts[fg, 1:3]
    assert np.abs(wrong - want).max() > 1.0                            # what a stride of 8 would have read
    emb = st['head'][:, 6:8].detach().cpu().numpy()[fg].astype(np.float64)
    d = np.abs(emb - want)
    sl1 = np.where(d < 1.0, 0.5 * d * d, d - 0.5).sum(1).mean()
    assert abs(tb['l_points_embed'] - sl1) <= 1e-5 * sl1, (tb['l_points_embed'], sl1)
    after = bd['gt_boxes'].cpu().numpy()
    assert after.shape == gt.shape and np.array_equal(after, _filter_numpy(gt, MINI_RANGE))
    assert any(not np.array_equal(after[b], gt[b]) for b in range(2))


def test_corrector_model_step_repeats_to_the_atomics_noise(mini, fp32_run):
    """the point <-> BEV backward kernels add with float atomics: a repeated first step gives the loss to 1e-6 relative and the gradients to
    1e-4 of their tensor's scale (the bounds of tests/test_gpu_train_e2e.py for two runs of the car model)"""
    la, _tb, ga = fp32_run[0][0]
    (lb, _tb2, gb), = _train_iterations(mini, 1)[0]
    assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)
    gmax = max(float(v.abs().max()) for v in ga.values())
    for n in ga:
        assert float((ga[n] - gb[n]).abs().max()) <= 1e-4 * max(float(ga[n].abs().max()), 1e-3 * gmax), n


def test_corrector_model_bf16_loop_tracks_the_fp32_loss(mini, fp32_run, monkeypatch):
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    (l16, _tb, g16), = _train_iterations(mini, 1)[0]
    l32 = fp32_run[0][0][0]
    print('bf16 loop loss %.6f, fp32 %.6f' % (l16, l32))
    assert np.isfinite(l16) and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert all(torch.isfinite(v).all() for v in g16.values())


def test_eval_after_a_step_repacks_the_corrector(mini):
    """eval() after an optimizer step gives the final sets of a fresh model loaded from the stepped state_dict(): HunterJr's packed weights,
    the fused point-head form included, were dropped by the training forward"""
    from pcdet.models import build_network_from_meta

    eval_points = load_golden('g24_corr_mini.npz')['points']     # the cloud this geometry's score threshold was set on: non-empty sets

    def final_sets(m):
        m.eval()
        assert m.corrector.fused_point_head
        bd = {'points': torch.from_numpy(eval_points.copy()).to(DEV), 'batch_size': 2, 'metadata': [{}, {}]}
        with torch.no_grad():
            preds, _ = m(bd)
        assert m.corrector.packed()['fused'] is not None
        return [dict(p, fused_map=bd['spatial_features_2d'][b].clone(), points=bd['points'].clone()) for b, p in enumerate(preds)]
    model, opt, sched, ocfg = _model_and_optimizer(mini['meta'])
    before = final_sets(model)                       # packs the UNSTEPPED weights first
    sched.step(0)
    model.train()
    opt.zero_grad()
    ret, _tb, _disp = model(_device_batch(mini['batch']))
    model.update_global_step()
    ret['loss'].backward()
    opt.clip_grad_norm(ocfg.GRAD_NORM_CLIP)
    opt.step()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    got = final_sets(model)
    fresh = build_network_from_meta(mini['meta'])
    fresh.load_state_dict(sd)
    want = final_sets(fresh.to(DEV))
    assert sum(p['pred_boxes'].shape[0] for p in got) > 0
    assert any(not torch.equal(a['fused_map'], b['fused_map']) for a, b in zip(got, before))       # the step moved the corrector's output
    for a, b in zip(got, want):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels', 'fused_map', 'points'):
            assert torch.equal(a[k], b[k]), k


def test_withmap_trains_on_the_loader_batch_and_ignores_instances_tf():
    g = load_golden('g20_nusc_mini.npz')
    meta = dict(g['meta']['cases']['withmap'])
    batch, cfg = _loader_batch('pointpillar_jr_withmap.yaml')
    meta['optimization'] = cfg.OPTIMIZATION
    meta['total_it_each_epoch'] = 5
    assert 'instances_tf' in batch and batch['gt_boxes'].shape[2] == 10
    losses = []
    for with_tf in (True, False):
        model, opt, sched, _ocfg = _model_and_optimizer(meta)
        sched.step(0)
        model.train()
        opt.zero_grad()
        bd = _device_batch(batch)
        if not with_tf:
            del bd['instances_tf']
        ret, tb, _disp = model(bd)
        ret['loss'].backward()
        grads = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
        assert all(v is not None and torch.isfinite(v).all() for v in grads.values())
        assert 'loss_corrector' not in tb
        losses.append(float(ret['loss'].detach()))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


def test_train_py_runs_the_corrector_config(tmp_path):
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'train.py', '--cfg_file', 'cfgs/nuscenes_models/pointpillar_jr_corr_withmap.yaml', '--batch_size', '2', '--epochs', '1',
           '--output_dir', str(tmp_path), '--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE),
           'DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME', '600', 'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '2', 'DATA_CONFIG.SYNTHETIC.XY_HALF', '6.5',
           'DATA_CONFIG.SYNTHETIC.DISTRIBUTION', 'uniform']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    losses = [float(m) for m in re.findall(r'loss ([0-9.]+)  lr', r.stdout + r.stderr)]
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses), (losses, (r.stdout + r.stderr)[-1500:])
    ck = torch.load(os.path.join(str(tmp_path), 'ckpt', 'checkpoint_epoch_1.pth'), map_location='cpu', weights_only=False)
    assert ck['epoch'] == 1 and ck['it'] == 1 and 'corrector.object_head.local_tf_decoder.0.weight' in ck['model_state']
    assert all(torch.isfinite(v).all() for v in ck['model_state'].values() if v.dtype.is_floating_point)
