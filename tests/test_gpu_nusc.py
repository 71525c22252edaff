"""nuScenes PointPillar-Jr models on the MI355X: the SC backbone's kernels (pool, gate, pre-activation residual 1x1) and the velocity
decode against torch-CPU fp32, the whole model against the reference's own outputs (tests/golden/g20_nusc_*.npz, written by
make_golden_nusc.py), and the graph replay against the eager forward."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_same_final_set, load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- ops --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W', [(30, 30), (15, 15), (22, 13), (64, 64)])
def test_avgpool_matches_torch(H, W):
    from pcp_amd import ops
    x = torch.randn(2, H, W, 40, generator=_gen(1))
    got = ops.avgpool_nhwc(x.cuda(), 4, in_ch_off=8, c=24)
    want = F.avg_pool2d(x[..., 8:32].permute(0, 3, 1, 2), 4, 4).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.allclose(got.cpu(), want, atol=1e-6, rtol=0)


@pytest.mark.parametrize('H,W', [(30, 30), (15, 15), (22, 13), (27, 30), (64, 64), (8, 8)])
@pytest.mark.parametrize('inplace', [False, True])
def test_sc_gate_matches_torch_interpolate(H, W, inplace):
    """sizes that are not 4 x the pooled size: torch's nearest index is min(floor(i * in / out), in - 1), not i // 4"""
    from pcp_amd import ops
    g = _gen(H * 100 + W)
    C = 32
    t = torch.randn(2, H, W, C + 8, generator=g)              # k3 output in a wider buffer (window at 4)
    xb = torch.randn(2, H, W, 2 * C, generator=g)             # the merged conv1_a | conv1_b map; x = window C..2C
    s = torch.randn(2, H // 4, W // 4, C, generator=g)
    want = t[..., 4:4 + C] * torch.sigmoid(
        xb[..., C:].permute(0, 3, 1, 2) + F.interpolate(s.permute(0, 3, 1, 2), size=(H, W))).permute(0, 2, 3, 1)
    tc, xc, sc = t.cuda(), xb.cuda(), s.cuda()
    if inplace:
        ops.sc_gate(tc, xc, sc, C, t_ch_off=4, x_ch_off=C)
        got = tc[..., 4:4 + C]
        assert torch.equal(tc[..., :4].cpu(), t[..., :4]) and torch.equal(tc[..., 4 + C:].cpu(), t[..., 4 + C:])
    else:
        out = torch.zeros(2, H, W, C + 4, device='cuda')
        ops.sc_gate(tc, xc, sc, C, t_ch_off=4, x_ch_off=C, out=out, out_ch_off=4)
        got = out[..., 4:]
    assert torch.allclose(got.cpu(), want, atol=1e-6, rtol=1e-6)


def test_pointwise_residual_before_relu():
    from pcp_amd import lib, ops, pack
    g = _gen(7)
    B, H, W, cin, cout = 2, 17, 19, 128, 256
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    r = torch.randn(B, H, W, cout, generator=g)
    wp, bp, cpad = pack.pack_plain(w.cuda(), b.cuda())
    got = ops.pointwise(x.cuda(), wp, bp, lib.PW_PLAIN, cin, cout, cpad, relu=True, residual=r.cuda(), residual_before_relu=True)
    want = torch.relu(x @ w.t() + b + r)
    assert torch.allclose(got.cpu(), want, atol=1e-5, rtol=0)
    # relu = 1 keeps its meaning: the residual after the activation
    got1 = ops.pointwise(x.cuda(), wp, bp, lib.PW_PLAIN, cin, cout, cpad, relu=True, residual=r.cuda())
    assert torch.allclose(got1.cpu(), torch.relu(x @ w.t() + b) + r, atol=1e-5, rtol=0)


def _scores_ref(head, kw, calib):
    nc = kw['num_class']
    hm = head[..., kw['ch_hm']:kw['ch_hm'] + nc].permute(0, 3, 1, 2).sigmoid()
    if calib:
        iou = head[..., kw['ch_iou']:kw['ch_iou'] + 1].permute(0, 3, 1, 2)
        hm = torch.pow(hm, 0.5) * torch.pow(torch.clamp((iou + 1) / 2.0, min=0.0, max=1.0), 0.5)
    return hm


def _mid_gap_threshold(head, kw, calib):
    """a score cut through the middle of the top-K list of every frame: the centre of the widest gap between ranks 100 and 400"""
    hm = _scores_ref(head, kw, calib)
    best = None
    for b in range(hm.shape[0]):
        top = np.sort(hm[b].reshape(-1).double().numpy())[::-1][100:400]
        i = int(np.argmax(top[:-1] - top[1:]))
        thr = float(np.float32((top[i] + top[i + 1]) / 2))
        best = thr if best is None else best
    return best


def _decode_reference(head, kw, calib):
    """centernet_utils.decode_bbox_from_heatmap (+ CALIB_CLS_SCORE) in torch-CPU fp32 on one NHWC head buffer; top-K as one sort over
    (class, cell) with ties to the lower flat index"""
    B, H, W, _ = head.shape
    hm = _scores_ref(head, kw, calib)
    out = []
    for b in range(B):
        flat = hm[b].reshape(-1)
        order = np.lexsort((np.arange(flat.numel()), -flat.double().numpy()))[:kw['k']]
        sc = flat[order]
        cell = torch.from_numpy(order % (H * W))
        px = head[b].reshape(H * W, -1)[cell]
        xs = (cell % W).float() + px[:, kw['ch_center']]
        ys = (cell // W).float() + px[:, kw['ch_center'] + 1]
        box = torch.stack([xs * kw['stride'] * kw['voxel_x'] + kw['min_x'], ys * kw['stride'] * kw['voxel_y'] + kw['min_y'],
                           px[:, kw['ch_z']], px[:, kw['ch_dim']].exp(), px[:, kw['ch_dim'] + 1].exp(), px[:, kw['ch_dim'] + 2].exp(),
                           torch.atan2(px[:, kw['ch_rot'] + 1], px[:, kw['ch_rot']])], 1)
        lim = kw['limit']
        m = (box[:, 0] >= lim[0]) & (box[:, 1] >= lim[1]) & (box[:, 2] >= lim[2]) & (box[:, 0] <= lim[3]) & (box[:, 1] <= lim[4]) \
            & (box[:, 2] <= lim[5]) & (sc > kw['score_thresh'])
        vel = px[:, kw['ch_vel']:kw['ch_vel'] + 2]
        full = np.sort(-flat.double().numpy())
        out.append(dict(boxes=box[m], scores=sc[m], flat=torch.from_numpy(order)[m], vel=vel[m], kgap=float(full[kw['k']] - full[kw['k'] - 1]),
                        tgap=float((sc.double() - kw['score_thresh']).abs().min())))
    return out


@pytest.mark.parametrize('calib', [False, True])
def test_decode_ext_two_class_128(calib):
    """2 classes x 128 x 128 = 32 768 candidates (over pcp_centerhead_decode's cap) for three heads in one launch, with vel: the exact
    candidate set, descending order (exact wherever two reference scores are more than 1e-6 apart), boxes to 1e-5, vel exact"""
    from pcp_amd import ops
    B, H, W, ld = 2, 128, 128, 16
    heads, kws = [], []
    for hi in range(3):
        g = _gen(100 + hi)
        buf = torch.randn(B, H, W, ld, generator=g) * 0.5
        # distinct logits: a permutation of an even grid
        perm = torch.randperm(2 * H * W, generator=g).float() / (2 * H * W) * 8.0 - 4.0
        buf[..., 12:14] = perm.reshape(H, W, 2).unsqueeze(0).expand(B, H, W, 2) + torch.arange(B).view(B, 1, 1, 1) * 1e-3
        buf[..., 11] = torch.rand(B, H, W, generator=g) * 1.8 - 0.9              # iou in (-0.9, 0.9): the clamp stays open
        kw = dict(k=500, num_class=2, ch_center=0, ch_z=2, ch_dim=3, ch_rot=6, ch_hm=12, stride=4.0, voxel_x=0.2, voxel_y=0.2,
                  min_x=-51.2, min_y=-51.2, limit=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], ch_vel=8)
        if calib:
            kw.update(ch_iou=11, iou_alpha=0.5)
        kw['score_thresh'] = _mid_gap_threshold(buf, kw, calib)
        heads.append(buf)
        kws.append(kw)
    res = ops.centerhead_decode_ext([(h.cuda(), kw) for h, kw in zip(heads, kws)])
    HW = H * W
    for h, kw, (boxes, scores, labels, cell, count, vel) in zip(heads, kws, res):
        for b, want in enumerate(_decode_reference(h, kw, calib)):
            assert want['kgap'] > 1e-6 and want['tgap'] > 1e-6, 'test input too close to the K cut / the score cut'
            n = int(count[b])
            assert n == want['boxes'].shape[0] and 8 <= n < kw['k']
            flat = (labels[b, :n].long() * HW + cell[b, :n].long()).cpu()
            assert set(flat.tolist()) == set(want['flat'].tolist())
            ws = want['scores']
            assert torch.allclose(scores[b, :n].cpu(), ws, atol=1e-6, rtol=0)
            distinct = torch.ones(n, dtype=torch.bool)
            close = (ws[:-1] - ws[1:]).abs() <= 1e-6
            distinct[:-1] &= ~close
            distinct[1:] &= ~close
            assert torch.equal(flat[distinct], want['flat'][distinct])
            pos = {int(f): i for i, f in enumerate(want['flat'].tolist())}
            idx = torch.tensor([pos[int(f)] for f in flat.tolist()])
            assert torch.allclose(boxes[b, :n].cpu(), want['boxes'][idx], atol=1e-5, rtol=1e-6)
            assert torch.equal(vel[b, :n].cpu(), want['vel'][idx])


def test_gather_ext_appends_vel_in_keep_order():
    from pcp_amd import ops
    g = _gen(3)
    B, k, km = 2, 40, 10
    heads, want = [], [[] for _ in range(B)]
    for hi in range(2):
        boxes, scores = torch.randn(B, k, 7, generator=g), torch.rand(B, k, generator=g)
        vel, labels = torch.randn(B, k, 2, generator=g), torch.randint(0, 2, (B, k), generator=g).int()
        keep = torch.stack([torch.randperm(k, generator=g)[:km] for _ in range(B)]).int()
        cnt = torch.tensor([7, 3], dtype=torch.int32)
        cmap = torch.tensor([3, 5], dtype=torch.int32) if hi else torch.tensor([0, 1], dtype=torch.int32)
        heads.append(dict(boxes=boxes.cuda(), scores=scores.cuda(), labels=labels.cuda(), keep=keep.cuda(), keep_count=cnt.cuda(),
                          class_map=cmap.cuda(), vel=vel.cuda()))
        for b in range(B):
            sel = keep[b, :int(cnt[b])].long()
            want[b].append((torch.cat([boxes[b, sel], vel[b, sel]], 1), scores[b, sel], cmap[labels[b, sel].long()].long() + 1))
    ob, os_, ol, oc = ops.gather_detections_ext(heads, B)
    for b in range(B):
        wb = torch.cat([w[0] for w in want[b]])
        n = wb.shape[0]
        assert int(oc[b]) == n and ob.shape[-1] == 9
        assert torch.equal(ob[b, :n].cpu(), wb)
        assert torch.equal(os_[b, :n].cpu(), torch.cat([w[1] for w in want[b]]))
        assert torch.equal(ol[b, :n].cpu(), torch.cat([w[2] for w in want[b]]))


# ---- model ------------------------------------------------------------------------------------------------------------------------

def _model(meta, iou_scale=None):
    from pcdet.models import build_network_from_meta
    state = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    if iou_scale is not None:
        state = {k: (v * np.float32(iou_scale) if '.iou.1.' in k else v) for k, v in state.items()}
    model = build_network_from_meta(meta).cuda().eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model


def _run(model, pts, batch_size):
    bd = {'points': torch.from_numpy(pts).cuda(), 'batch_size': batch_size, 'metadata': [{}] * batch_size}
    with torch.no_grad():
        preds, _ = model(bd)
    torch.cuda.synchronize()
    return bd, preds


@pytest.mark.parametrize('algo', ['auto', 'direct'])
def test_mini_backbone_and_head_maps_match_the_reference(algo, monkeypatch):
    if algo != 'auto':
        monkeypatch.setenv('PCP_CONV_ALGO', algo)
    g = load_golden('g20_nusc_mini.npz')
    model = _model(g['meta']['cases']['nomap'])
    bd, _ = _run(model, g['points'], 2)
    sf = bd['spatial_features_2d'].cpu().numpy()
    assert sf.shape == g['spatial_features_2d'].shape
    err = float(np.abs(sf - g['spatial_features_2d']).max())
    assert err < 1e-3, err
    pds = model.dense_head.forward_ret_dict['pred_dicts']
    assert len(pds) == 6
    for h, pd in enumerate(pds):
        for name, v in pd.items():
            want = g['head%d_%s' % (h, name)]
            e = float(np.abs(v.cpu().numpy() - want).max())
            assert e < 1e-3, (h, name, e)


@pytest.mark.parametrize('case,points_key', [('nomap', 'points'), ('withmap', 'points_map'), ('calib', 'points')])
def test_mini_final_sets_are_the_reference_ones(case, points_key):
    g = load_golden('g20_nusc_mini.npz')
    meta = g['meta']['cases'][case]
    model = _model(meta, meta.get('iou_scale'))
    _bd, preds = _run(model, g[points_key], 2)
    for b in range(2):
        got_b = preds[b]['pred_boxes'].cpu().numpy()
        assert got_b.shape[1] == 9
        assert_same_final_set(g['%s_boxes_%d' % (case, b)], g['%s_scores_%d' % (case, b)], got_b, preds[b]['pred_scores'].cpu().numpy(),
                              tol=1e-3)
        # labels: 1-based global class ids through class_id_mapping_each_head, the same multiset as the reference's
        assert sorted(preds[b]['pred_labels'].cpu().numpy().tolist()) == sorted(g['%s_labels_%d' % (case, b)].tolist())


def _full_points(meta):
    c = meta['cloud']
    pts = synth.collate([synth.nusc_cloud(b, c['points_per_frame'], c['xy_half']) for b in range(c['frames'])])
    assert hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest() == meta['points_sha256']
    return pts


def test_full_b4_probes_and_final_set():
    g = load_golden('g20_nusc_full_b4.npz')
    meta = g['meta']['cases']['nomap']
    pts = _full_points(meta)
    model = _model(meta)
    bd, preds = _run(model, pts, 4)
    p, c = meta['probe_pix'], meta['probe_sf_ch']
    sf = bd['spatial_features_2d'][:, ::c, ::p, ::p].cpu().numpy()
    assert float(np.abs(sf - g['sf_probe']).max()) < 1e-3
    for h, pd in enumerate(model.dense_head.forward_ret_dict['pred_dicts']):
        for name, v in pd.items():
            e = float(np.abs(v[:, :, ::p, ::p].cpu().numpy() - g['head%d_%s_probe' % (h, name)]).max())
            assert e < 1e-3, (h, name, e)
    for b in range(4):
        assert_same_final_set(g['nomap_boxes_%d' % b], g['nomap_scores_%d' % b], preds[b]['pred_boxes'].cpu().numpy(),
                              preds[b]['pred_scores'].cpu().numpy(), tol=1e-3)


def test_graph_replay_is_bitwise_the_eager_forward():
    from pcdet.models.graphed import GraphedDetector
    g = load_golden('g20_nusc_mini.npz')
    model = _model(g['meta']['cases']['nomap'])
    pts = torch.from_numpy(g['points']).cuda()
    _bd, eager = _run(model, g['points'], 2)
    gd = GraphedDetector(model, pts, 2, [{}, {}])
    got = gd(pts)
    torch.cuda.synchronize()
    for b in range(2):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(got[b][k], eager[b][k]), (b, k)
        assert got[b]['pred_boxes'].shape[1] == 9


def test_pipelined_runner_keeps_the_velocity_columns():
    from pcdet.models.pipelined import PipelinedDetector
    g = load_golden('g20_nusc_mini.npz')
    model = _model(g['meta']['cases']['nomap'])
    _bd, eager = _run(model, g['points'], 2)
    assert PipelinedDetector.supports(model)
    runner = PipelinedDetector(model)
    pts = torch.from_numpy(g['points']).cuda()
    assert runner.submit(pts, 2, [{}, {}]) is None
    got = runner.flush()
    torch.cuda.synchronize()
    for b in range(2):
        assert got[b]['pred_boxes'].shape[1] == 9
        assert torch.equal(got[b]['pred_boxes'], eager[b]['pred_boxes'])
        assert torch.equal(got[b]['pred_scores'], eager[b]['pred_scores'])
