"""v2x_second_car / v2x_second_rsu on the MI355X: the fused point-head kernel at 256 channels (hidden 32 and 64) against the sampling
kernel, the unfused HIP chain and a float64 restatement; the channel window HunterJr reads it through; the refusals; HunterJr alone at
this width against the reference's own outputs (tests/golden/g30_second_corr_module.npz, written by make_golden_second_corr.py); the two
whole models at a mini range, their exchange files, and tools/test.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import second_corr_refs as R
from helpers import assert_same_final_set, load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
C = 256
YAMLS = {'car': 'cfgs/v2x_sim_models/v2x_second_car.yaml', 'rsu': 'cfgs/v2x_sim_models/v2x_second_rsu.yaml'}
# 128 x 128 x 40 voxels of (0.1, 0.1, 0.2) with the z-extent of each YAML (car overrides it to -5 .. 3)
MINI_RANGE = {'car': [-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], 'rsu': [-6.4, -6.4, -8.0, 6.4, 6.4, 0.0]}


# ---- the kernel at C = 256 ------------------------------------------------------------------------------------------------------------

def _fused(c, flow, order, bev=None, channels=C):
    from pcp_amd import ops
    bev = torch.from_numpy(c['bev']).cuda() if bev is None else bev
    pts = torch.from_numpy(c['points'].copy()).cuda()
    od = None
    if order:
        # a permutation of the rows that is not the identity: results must land at the original rows
        od = torch.from_numpy(np.ascontiguousarray(np.arange(pts.shape[0])[::-1].astype(np.int32))).cuda()
    r = ops.hunter_point_head(bev, pts, R.MIN_XY, R.PIX, *R.weights_cuda(c), channels=channels, order=od,
                              flow_thresh=R.THRESH if flow else None)
    torch.cuda.synchronize()
    return r, bev, pts


@pytest.mark.parametrize('flow', [False, True])
@pytest.mark.parametrize('order', [False, True])
@pytest.mark.parametrize('n', R.NS)
@pytest.mark.parametrize('hidden', R.HIDDEN)
def test_point_head_256(hidden, n, order, flow):
    """N straddles the 32-point tile; rows of no frame (batch index -1) and rows outside the map are in; with and without a visiting
    order; pcp_hunter_point_head (no order, no flow) and pcp_hunter_point_head_ex (the rest).  Fails without the 256-channel
    instantiations: the call returns PCP_ERR_UNSUPPORTED.  The two head8 bars are those of test_gpu_nusc_corr.py at K = 384.
    Measured on the MI355X over all 40 cases: |head8 - unfused chain| <= 9.54e-7, |head8 - float64| <= 4.77e-7."""
    from pcp_amd import ops
    c = R.case(C, hidden, n)
    r, bev, pts = _fused(c, flow, order)
    pf, head8 = r[0], r[1]
    before = torch.from_numpy(c['points']).cuda()
    want_pf = ops.bev_sample_bilinear(bev, before, R.MIN_XY, R.PIX, out=torch.zeros((n, C), device='cuda'), channels=C)   # rows of no frame: 0
    first_pf = want_pf.clone()
    none = before[:, 0] < 0
    if flow:
        # dyn and the moved points are k_apply_flow's on the kernel's own head values; corrected rows are re-sampled where they went
        moved = before.clone()
        want_dyn = ops.hunter_apply_flow(moved, head8, R.THRESH)
        assert torch.equal(r[2], want_dyn)
        assert torch.equal(pts, moved)
        if n >= 31:
            assert 0 < int(want_dyn.sum()) < n
        ops.bev_sample_bilinear(bev, moved, R.MIN_XY, R.PIX, out=want_pf, row_mask=want_dyn, channels=C)
    else:
        assert torch.equal(pts, before)
    assert torch.equal(pf, want_pf)                                              # bit-equal to the sampling kernel
    assert not pf[none].any()                                                    # rows of no frame: exactly 0
    c_pf, c_head8, c_dyn, c_after = R.unfused_chain(c, flow)
    err = float((head8.cpu() - c_head8).abs().max())
    print('C 256 hidden %d n %d order %s flow %s: |head8 - unfused chain| = %.3g' % (hidden, n, order, flow, err), end='')
    ref = R.head8_torch(c, first_pf.cpu())
    err_t = float((head8.cpu() - ref).abs().max())
    print(', |head8 - float64| = %.3g' % err_t)
    assert err < 1e-4, err
    assert R.verdict_margin(ref) > 1e-3, 'test input too close to a dynamic-foreground verdict'
    assert err_t < 1e-3, err_t
    if flow:
        assert torch.equal(r[2].cpu(), c_dyn)
        assert float((pts.cpu() - c_after).abs().max()) < 1e-4                  # the chain moved its rows by ITS head values


@pytest.mark.parametrize('flow', [False, True])
@pytest.mark.parametrize('hidden', R.HIDDEN)
def test_point_head_256_reads_a_channel_window(hidden, flow):
    """the way HunterJr calls the kernel: the map is the first 256 channels of a 512-wide [bev | corrected] buffer (ld_bev = 512,
    bev_ch_off = 0).  Every output is bit-equal to the one from a contiguous 256-wide copy"""
    c = R.case(C, hidden, 97)
    wide = torch.full((R.B, R.H, R.W, 2 * C), 7.0, device='cuda')               # the second half must never be read
    wide[..., :C] = torch.from_numpy(c['bev']).cuda()
    r_w, _bev, pts_w = _fused(c, flow, True, bev=wide)
    r_c, _bev, pts_c = _fused(c, flow, True)
    assert wide.shape[3] == 512 and len(r_w) == len(r_c) == (3 if flow else 2)
    for a, b in zip(r_w, r_c):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(pts_w, pts_c)
    assert r_w[0].shape == (97, C)


def test_point_head_rejects_other_widths():
    from pcp_amd import ops
    from pcp_amd.lib import PcpError
    for channels in (128, 320):
        c = R.case(channels, 32, 8)
        bev, pts = torch.from_numpy(c['bev']).cuda(), torch.from_numpy(c['points']).cuda()
        with pytest.raises(PcpError):
            ops.hunter_point_head(bev, pts, R.MIN_XY, R.PIX, *R.weights_cuda(c), channels=channels)
    c = R.case(C, 64, 8)
    w1, b1, w2, b2, wh, bh = R.weights_cuda(c)
    bev, pts = torch.from_numpy(c['bev']).cuda(), torch.from_numpy(c['points']).cuda()
    with pytest.raises(PcpError):
        ops.hunter_point_head(bev, pts, R.MIN_XY, R.PIX, w1[:48].contiguous(), b1[:48].contiguous(), w2[:, :48].contiguous(), b2, wh, bh,
                              channels=C)


# ---- HunterJr alone against the reference -------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden():
    return load_golden('g30_second_corr_module.npz')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('hidden', [32, 64])
def test_module_matches_the_reference_hunter_jr(golden, hidden, fused):
    """conv_input 256 -> 256, the point head, bev_scatter_mean and softmax_fuse_raw on the 512-wide buffer, the weightor's 512 -> 512 conv
    and the 512 -> 2 conv through conv3x3_grouped_small, against the reference's HunterJr on the CPU.  Bars of
    test_gpu_nusc_corr.py::test_module_matches_the_reference_hunter_jr.  Measured on the MI355X, largest of fused and chain, hidden 32 /
    64: |head8| err 5.5e-6 / 6.2e-6, |map| err 8.3e-6 / 7.4e-6, corrected rows err 3.8e-6 / 5.7e-6."""
    from pcdet.config import EasyDict
    from pcdet.models.bev_layers.hunter_jr import HunterJr
    g, t = golden, 'h%d_' % hidden
    meta, case = g['meta'], g['meta']['cases'][str(hidden)]
    state = synth.fill_state_dict(case['state_shapes'], scheme=meta['weight_scheme'])
    for k, v in case['state_overrides'].items():
        state[k] = np.asarray(v, dtype=np.float32)
    corr = HunterJr(EasyDict(case['corrector']), meta['num_bev_features'], meta['voxel_size'], meta['pc_range'])
    corr.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    corr = corr.cuda().eval()
    corr.keep_point_heads = True
    corr.fused_point_head = fused
    pk = corr.packed()
    assert (pk['fused'] is not None) and tuple(pk['fused'][0].shape) == (hidden, 256)
    assert pk['w1_small'] is not None and tuple(pk['w1_small'][0].shape) == (2, 9, 512)
    m = meta['map']
    x = synth.uniform(m['seed'], m['stream'], int(np.prod(m['shape'])), m['lo'], m['hi']).reshape(m['shape'])
    bd = {'points': torch.from_numpy(g['points'].copy()).cuda(), 'spatial_features_2d': torch.from_numpy(x).cuda(), 'batch_size': 2,
          'metadata': [{}, {}]}
    with torch.no_grad():
        bd = corr(bd)
    torch.cuda.synchronize()
    assert 'scene_flow' not in bd
    assert bd['spatial_features_2d'].shape == (2, 256, 12, 12)
    e_head = float(np.abs(bd['hunter_point_heads'].cpu().numpy() - g[t + 'head8']).max())
    e_map = float(np.abs(bd['spatial_features_2d'].cpu().numpy() - g[t + 'spatial_features_2d']).max())
    after = bd['points'].cpu().numpy()
    dyn = g[t + 'dyn'].astype(bool)
    e_pts = float(np.abs(after[dyn] - g[t + 'points_after'][dyn]).max())
    print('module hidden %d (fused %s): |head8| err %.3g, |map| err %.3g, corrected rows err %.3g' % (hidden, fused, e_head, e_map, e_pts))
    assert e_head < 1e-3, e_head
    assert np.array_equal(after[~dyn], g['points'][~dyn])                        # untouched rows: bit-equal (this IS the exact mask)
    assert (np.abs(after[dyn, 1:4] - g['points'][dyn, 1:4]).max(1) > 0).all()
    assert e_pts < 1e-5, e_pts
    assert e_map < 1e-3, e_map


# ---- the whole models -----------------------------------------------------------------------------------------------------------------

def _mini_model(which, exchange_dir):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import SyntheticV2XDataset
    from pcdet.models import build_network
    cwd = os.getcwd()
    os.chdir(os.path.join(PKG, 'tools'))
    try:
        cfg = cfg_from_yaml_file(YAMLS[which], EasyDict())
    finally:
        os.chdir(cwd)
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE[which])
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=4000, NUM_FRAMES=3, DISTRIBUTION='uniform')
    cfg.MODEL.CORRECTOR.DATABASE_EXCHANGE_DATA = str(exchange_dir)
    cfg.MODEL.DENSE_HEAD.DATABASE_EXCHANGE_DATA = str(exchange_dir)
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval(), ds


def _preds(model, ds):
    from pcdet.models import load_data_to_gpu
    batch = ds.collate_batch([ds[i] for i in range(3)])
    load_data_to_gpu(batch)
    with torch.no_grad():
        pred, _ = model(batch)
    torch.cuda.synchronize()
    return [(p['pred_boxes'].cpu().numpy(), p['pred_scores'].cpu().numpy(), p['pred_labels'].cpu().numpy()) for p in pred], batch


GAP = 1e-3          # no verdict of the conditioned model within half of this of flipping: a thousand times the kernels' measured difference


def _widest_gap(v):
    """(middle, width) of the widest gap of the values between the 0.5 % and 99.5 % ranks"""
    v = torch.sort(v)[0]
    a, b = max(1, int(0.005 * len(v))), len(v) - 1 - max(1, int(0.005 * len(v)))
    k = a + int(torch.argmax(v[a + 1:b + 1] - v[a:b]))
    return float((v[k] + v[k + 1]) / 2), float(v[k + 1] - v[k])


def _condition_seg_bias(model, ds):
    """the synthetic weights decide nothing about which rows are foreground: as the fixture generator does, the class biases are moved so
    that a cut falls into a gap of the sorted logits -- the background logit for the rows that are sent (sigmoid(background) < 0.3), then
    the dynamic logit for the rows that are corrected.  The widest gap is taken wherever it lies: the rows outside the mini map (most of
    the synthetic cloud) sample clamped corners whose weights cancel, so their logits form one tight cluster that no cut may split"""
    corr = model.corrector
    corr.keep_point_heads = True
    _p, batch = _preds(model, ds)
    head = batch['hunter_point_heads'].double().cpu()
    cut = float(np.log(0.3 / 0.7))
    mid0, gap0 = _widest_gap(head[:, 0])
    l0 = head[:, 0] + (cut - mid0)
    mid2, gap2 = _widest_gap(head[:, 2] - torch.clamp(torch.maximum(l0, head[:, 1]), min=cut))
    assert gap0 > GAP and gap2 > GAP, (gap0, gap2)
    with torch.no_grad():
        corr.point_head.seg[0].bias[0] += cut - mid0
        corr.point_head.seg[0].bias[2] -= mid2
    corr.invalidate_packed()


@pytest.mark.parametrize('which', ['car', 'rsu'])
def test_whole_model_runs_repeats_and_writes_exchange_data(which, tmp_path):
    model, ds = _mini_model(which, tmp_path)
    assert [type(m).__name__ for m in model.module_list] == ['DynamicMeanVFE', 'VoxelResBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                              'HunterJr', 'CenterHead']
    assert list(ds.grid_size) == [128, 128, 40]
    hidden = 32 if which == 'car' else 64
    assert tuple(model.corrector.packed()['fused'][0].shape) == (hidden, 256) and model.corrector.fused_point_head
    _condition_seg_bias(model, ds)
    for f in os.listdir(tmp_path):
        os.remove(os.path.join(tmp_path, f))
    full, batch = _preds(model, ds)
    assert batch['spatial_features_2d'].shape == (3, 256, 16, 16) and batch['spatial_features'].shape == (3, 256, 16, 16)
    assert batch['voxel_features'].shape[1] == 5 and batch['points'].shape[1] == 8
    for boxes, scores, labels in full:
        assert boxes.ndim == 2 and boxes.shape[1] == 7 and np.isfinite(boxes).all() and np.isfinite(scores).all()
    # exchange data: car writes, rsu does not
    head8, pts = batch['hunter_point_heads'].cpu(), batch['points'].cpu()
    sent = torch.sigmoid(head8[:, 0]) < 0.3
    dynamic = R.dynamic_rows(head8)
    assert 0.0 < float(sent.float().mean()) < 1.0 and 0.0 < float(dynamic.float().mean()) < 1.0
    written = sorted(os.listdir(tmp_path))
    if which == 'rsu':
        assert written == []
    else:
        want = []
        for b, meta in enumerate(batch['metadata']):
            rows = sent & (pts[:, 0] == b)
            stem = '%s_id%s' % (meta['sample_token'], meta['lidar_id'])
            if int(rows.sum()) == 0:
                continue
            fg = torch.load(os.path.join(tmp_path, stem + '_foreground.pth'), map_location='cpu')
            assert tuple(fg.shape) == (int(rows.sum()), 13)
            assert torch.equal(fg[:, :7], pts[rows][:, 1:])                      # the point columns without the frame index, xyz as corrected
            assert torch.equal(fg[:, 10:13], head8[rows][:, 3:6])
            assert float((fg[:, 7:10] - torch.sigmoid(head8[rows][:, :3])).abs().max()) < 1e-6
            want.append(stem + '_foreground.pth')
            if full[b][0].shape[0]:
                mo = torch.load(os.path.join(tmp_path, stem + '_modar.pth'), map_location='cpu')
                assert mo.ndim == 2 and mo.shape[1] == 9 and 0 < mo.shape[0] <= 83 and mo.shape[0] == full[b][0].shape[0]
                want.append(stem + '_modar.pth')
        assert written == sorted(want)
        assert any(w.endswith('_foreground.pth') for w in want) and any(w.endswith('_modar.pth') for w in want)
    # a second run is bit-equal
    again, _ = _preds(model, ds)
    for a, b in zip(full, again):
        for u, v in zip(a, b):
            assert u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8))
    # the five-launch chain gives the same final sets
    model.corrector.fused_point_head = False
    chain, batch_u = _preds(model, ds)
    assert torch.equal(R.dynamic_rows(batch_u['hunter_point_heads'].cpu()), dynamic)
    for a, b in zip(full, chain):
        assert_same_final_set(a[0], a[1], b[0], b[1], tol=1e-4)
        assert sorted(a[2].tolist()) == sorted(b[2].tolist())


def test_refusals_of_the_whole_model(tmp_path):
    from pcdet.models.pipelined import PipelinedDetector
    model, _ds = _mini_model('car', tmp_path)
    with pytest.raises(NotImplementedError, match='inference only'):
        model.train()
    model.eval()
    assert not PipelinedDetector.supports(model)


# ---- command line -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('extra', [[], ['--fast']])
@pytest.mark.parametrize('which', ['car', 'rsu'])
def test_tools_test_py_runs_the_yaml(which, extra, tmp_path):
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', YAMLS[which], '--batch_size', '2'] + extra + \
          ['--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE[which]), 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '3000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '3', 'MODEL.CORRECTOR.DATABASE_EXCHANGE_DATA', str(tmp_path),
           'MODEL.DENSE_HEAD.DATABASE_EXCHANGE_DATA', str(tmp_path)]
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    out = r.stdout + r.stderr
    assert 'over 3 frames' in out, out[-1500:]
    if which == 'rsu':
        assert os.listdir(tmp_path) == []
