"""pointpillar_jr_corr_withmap on the MI355X: the fused point-head kernel at hidden width 64 (and, unchanged, 32) against the sampling
kernel, the unfused HIP chain and a torch-CPU restatement; HunterJr alone and the whole model against the reference's own outputs
(tests/golden/g24_corr_*.npz, written by make_golden_nusc_corr.py); the model with the fused kernel off, through PipelinedDetector, and
through tools/test.py."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nusc_corr_refs as R
from helpers import assert_same_final_set, load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


# ---- the kernel -------------------------------------------------------------------------------------------------------------------

def _fused(c, flow, order):
    from pcp_amd import ops
    bev, pts = torch.from_numpy(c['bev']).cuda(), torch.from_numpy(c['points'].copy()).cuda()
    od = None
    if order:
        # a permutation of the rows that is not the identity: results must land at the original rows
        od = torch.from_numpy(np.ascontiguousarray(np.arange(pts.shape[0])[::-1].astype(np.int32))).cuda()
    r = ops.hunter_point_head(bev, pts, R.MIN_XY, R.PIX, *R.weights_cuda(c), channels=R.C, order=od, flow_thresh=R.THRESH if flow else None)
    torch.cuda.synchronize()
    return r, bev, pts


@pytest.mark.parametrize('flow', [False, True])
@pytest.mark.parametrize('order', [False, True])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 97])
def test_point_head_hidden_64(n, order, flow):
    """N straddles the 32-point tile; rows of no frame (batch index -1) and rows outside the map are in; with and without a visiting
    order; pcp_hunter_point_head (no order, no flow) and pcp_hunter_point_head_ex (the rest).  Fails without the hidden-64
    instantiation: the call returns PCP_ERR_UNSUPPORTED."""
    from pcp_amd import ops
    c = R.case(64, n)
    r, bev, pts = _fused(c, flow, order)
    pf, head8 = r[0], r[1]
    before = torch.from_numpy(c['points']).cuda()
    want_pf = ops.bev_sample_bilinear(bev, before, R.MIN_XY, R.PIX, out=torch.zeros((n, R.C), device='cuda'), channels=R.C)   # rows of no frame: 0
    first_pf = want_pf.clone()
    if flow:
        # dyn and the moved points are k_apply_flow's on the kernel's own head values; corrected rows are re-sampled where they went
        moved = before.clone()
        want_dyn = ops.hunter_apply_flow(moved, head8, R.THRESH)
        assert torch.equal(r[2], want_dyn)
        assert torch.equal(pts, moved)
        if n >= 31:
            assert 0 < int(want_dyn.sum()) < n
        ops.bev_sample_bilinear(bev, moved, R.MIN_XY, R.PIX, out=want_pf, row_mask=want_dyn, channels=R.C)
    else:
        assert torch.equal(pts, before)
    assert torch.equal(pf, want_pf)                                              # bit-equal to the sampling kernel
    c_pf, c_head8, c_dyn, c_after = R.unfused_chain(c, flow)
    err = float((head8.cpu() - c_head8).abs().max())
    print('hidden 64 n %d order %s flow %s: |head8 - unfused chain| = %.3g' % (n, order, flow, err), end='')
    assert err < 1e-4, err
    ref = R.head8_torch(c, first_pf.cpu())
    assert R.verdict_margin(ref) > 1e-3, 'test input too close to a dynamic-foreground verdict'
    err_t = float((head8.cpu() - ref).abs().max())
    print(', |head8 - torch| = %.3g' % err_t)
    assert err_t < 1e-3, err_t
    if flow:
        assert torch.equal(r[2].cpu(), c_dyn)
        assert float((pts.cpu() - c_after).abs().max()) < 1e-4                  # the chain moved its rows by ITS head values


def test_point_head_rejects_other_widths():
    from pcp_amd import ops
    from pcp_amd.lib import PcpError
    c = R.case(64, 8)
    w1, b1, w2, b2, wh, bh = R.weights_cuda(c)
    bev, pts = torch.from_numpy(c['bev']).cuda(), torch.from_numpy(c['points']).cuda()
    with pytest.raises(PcpError):
        ops.hunter_point_head(bev, pts, R.MIN_XY, R.PIX, w1[:48].contiguous(), b1[:48].contiguous(), w2[:, :48].contiguous(), b2, wh, bh,
                              channels=R.C)


@pytest.mark.parametrize('flow', [False, True])
def test_point_head_hidden_32_keeps_its_bits(flow):
    """g24_ph32.npz: the head values, the moved points and the digest of the sampled rows that the fused kernel gave at hidden 32 BEFORE it
    became a template (recorded on an MI355X, same inputs), and the unfused chain's head values recorded beside them"""
    g = load_golden('g24_ph32.npz')
    tag = 'flow' if flow else 'plain'
    c = R.case(32, 97)
    r, _bev, pts = _fused(c, flow, False)
    assert float(np.abs(r[1].cpu().numpy() - g['chain_%s_head8' % tag]).max()) < 1e-4
    assert np.array_equal(r[1].cpu().numpy(), g['fused_%s_head8' % tag])
    assert _sha(r[0]) == str(g['fused_%s_pf_sha256' % tag])
    if flow:
        assert np.array_equal(r[2].cpu().numpy(), g['fused_flow_dyn'])
        assert np.array_equal(pts.cpu().numpy(), g['fused_flow_points_after'])
    else:
        assert _sha(r[0]) == str(g['chain_plain_pf_sha256'])


# ---- HunterJr alone -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fused', [True, False])
def test_module_matches_the_reference_hunter_jr(fused):
    from pcdet.config import EasyDict
    from pcdet.models.bev_layers.hunter_jr import HunterJr
    g = load_golden('g24_corr_module.npz')
    meta = g['meta']
    state = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    for k, v in meta['state_overrides'].items():
        state[k] = np.asarray(v, dtype=np.float32)
    corr = HunterJr(EasyDict(meta['corrector']), meta['num_bev_features'], meta['voxel_size'], meta['pc_range'])
    corr.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    corr = corr.cuda().eval()
    corr.keep_point_heads = True
    corr.fused_point_head = fused
    assert (corr.packed()['fused'] is not None) and tuple(corr.packed()['fused'][0].shape) == (64, 384)
    m = meta['map']
    x = synth.uniform(m['seed'], m['stream'], int(np.prod(m['shape'])), m['lo'], m['hi']).reshape(m['shape'])
    bd = {'points': torch.from_numpy(g['points'].copy()).cuda(), 'spatial_features_2d': torch.from_numpy(x).cuda(), 'batch_size': 2,
          'metadata': [{}, {}]}
    with torch.no_grad():
        bd = corr(bd)
    torch.cuda.synchronize()
    assert 'scene_flow' not in bd                                                # no exchange data unless asked for
    e_head = float(np.abs(bd['hunter_point_heads'].cpu().numpy() - g['head8']).max())
    e_map = float(np.abs(bd['spatial_features_2d'].cpu().numpy() - g['spatial_features_2d']).max())
    after = bd['points'].cpu().numpy()
    dyn = g['dyn'].astype(bool)
    e_pts = float(np.abs(after[dyn] - g['points_after'][dyn]).max())
    print('module (fused %s): |head8| err %.3g, |map| err %.3g, corrected rows err %.3g' % (fused, e_head, e_map, e_pts))
    assert e_head < 1e-3, e_head
    assert np.array_equal(after[~dyn], g['points'][~dyn])                        # untouched rows: bit-equal (this IS the exact mask)
    assert (np.abs(after[dyn, 1:4] - g['points'][dyn, 1:4]).max(1) > 0).all()
    assert e_pts < 1e-5, e_pts
    assert e_map < 1e-3, e_map


# ---- the whole model ------------------------------------------------------------------------------------------------------------------

def _model(meta):
    from pcdet.models import build_network_from_meta
    state = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    for k, v in meta['state_overrides'].items():
        state[k] = np.asarray(v, dtype=np.float32)
    model = build_network_from_meta(meta).cuda().eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model


def _run(model, pts, batch_size):
    bd = {'points': torch.from_numpy(pts.copy()).cuda(), 'batch_size': batch_size, 'metadata': [{}] * batch_size}
    with torch.no_grad():
        preds, _ = model(bd)
    torch.cuda.synchronize()
    return bd, preds


def _check_sets(g, preds, batch_size):
    for b in range(batch_size):
        got = preds[b]['pred_boxes'].cpu().numpy()
        assert got.shape[1] == 9
        assert_same_final_set(g['corr_boxes_%d' % b], g['corr_scores_%d' % b], got, preds[b]['pred_scores'].cpu().numpy(), tol=1e-3)
        assert sorted(preds[b]['pred_labels'].cpu().numpy().tolist()) == sorted(g['corr_labels_%d' % b].tolist())


def _pipelined(model, pts, batch_size):
    from pcdet.models.pipelined import PipelinedDetector
    assert PipelinedDetector.supports(model)
    runner = PipelinedDetector(model, replicas=2)
    out = []
    bufs = [torch.from_numpy(pts.copy()).cuda() for _ in range(2)]              # the corrector moves the points of the buffer it is given
    for buf in bufs:
        prev = runner.submit(buf, batch_size, [{}] * batch_size)
        if prev is not None:
            out.append(prev)
    out.append(runner.flush())
    torch.cuda.synchronize()
    return out


def test_mini_model_matches_the_reference():
    g = load_golden('g24_corr_mini.npz')
    meta = g['meta']['cases']['corr']
    model = _model(meta)
    assert model.corrector.fused_point_head and model.corrector.packed()['fused'] is not None
    bd, preds = _run(model, g['points'], 2)
    e = float(np.abs(bd['spatial_features_2d'].cpu().numpy() - g['spatial_features_2d']).max())
    assert e < 1e-3, e
    pds = model.dense_head.forward_ret_dict['pred_dicts']
    assert len(pds) == 6
    for h, pd in enumerate(pds):
        for name, v in pd.items():
            eh = float(np.abs(v.cpu().numpy() - g['head%d_%s' % (h, name)]).max())
            assert eh < 1e-3, (h, name, eh)
    dyn = g['dyn'].astype(bool)
    after = bd['points'].cpu().numpy()
    assert np.array_equal(after[~dyn], g['points'][~dyn])
    assert (np.abs(after[dyn, 1:4] - g['points'][dyn, 1:4]).max(1) > 0).all()
    assert float(np.abs(after[dyn] - g['points_after'][dyn]).max()) < 1e-5
    _check_sets(g, preds, 2)
    # the five-launch chain gives the same final set
    model.corrector.fused_point_head = False
    _bd, preds_u = _run(model, g['points'], 2)
    _check_sets(g, preds_u, 2)
    for b in range(2):
        assert_same_final_set(preds[b]['pred_boxes'].cpu().numpy()[:, :7], preds[b]['pred_scores'].cpu().numpy(),
                              preds_u[b]['pred_boxes'].cpu().numpy()[:, :7], preds_u[b]['pred_scores'].cpu().numpy(), tol=1e-4)
    model.corrector.fused_point_head = True
    for got in _pipelined(model, g['points'], 2):
        _check_sets(g, got, 2)
        for b in range(2):
            assert torch.equal(got[b]['pred_boxes'], preds[b]['pred_boxes']) and torch.equal(got[b]['pred_scores'], preds[b]['pred_scores'])


def test_full_geometry_probes_and_final_set():
    g = load_golden('g24_corr_full.npz')
    meta = g['meta']['cases']['corr']
    c = meta['cloud']
    pts = synth.collate([synth.nusc_cloud(b, c['points_per_frame'], c['xy_half'], c['with_map']) for b in range(c['frames'])])
    assert hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest() == meta['points_sha256']
    model = _model(meta)
    bd, preds = _run(model, pts, 1)
    p, ch = meta['probe_pix'], meta['probe_sf_ch']
    e = float(np.abs(bd['spatial_features_2d'][:, ::ch, ::p, ::p].cpu().numpy() - g['sf_probe']).max())
    assert e < 1e-3, e
    for h, pd in enumerate(model.dense_head.forward_ret_dict['pred_dicts']):
        for name, v in pd.items():
            eh = float(np.abs(v[:, :, ::p, ::p].cpu().numpy() - g['head%d_%s_probe' % (h, name)]).max())
            assert eh < 1e-3, (h, name, eh)
    dyn = np.unpackbits(g['dyn'])[:pts.shape[0]].astype(bool)
    after = bd['points'].cpu().numpy()
    assert np.array_equal(after[~dyn], pts[~dyn])
    assert (np.abs(after[dyn, 1:4] - pts[dyn, 1:4]).max(1) > 0).all()
    assert float(np.abs(after[dyn] - g['points_after_dyn']).max()) < 1e-5
    _check_sets(g, preds, 1)
    model.corrector.fused_point_head = False
    _bd, preds_u = _run(model, pts, 1)
    _check_sets(g, preds_u, 1)
    model.corrector.fused_point_head = True
    for got in _pipelined(model, pts, 1):
        _check_sets(g, got, 1)


# ---- command line ---------------------------------------------------------------------------------------------------------------------

def test_tools_test_py_runs_the_corrector_config():
    import re
    tools = os.path.join(REPO, 'practical-collab-perception_amd', 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', 'cfgs/nuscenes_models/pointpillar_jr_corr_withmap.yaml', '--batch_size', '1', '--set',
           'DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME', '20000', 'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '1']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    out = r.stdout + r.stderr
    assert 'Performance of EPOCH' in out
    m = re.search(r'(\d+) detections over (\d+) frames', out)
    assert m is not None and int(m.group(2)) == 1, out[-1500:]
