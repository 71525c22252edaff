"""CenterHead training with several heads, velocity codes and the IoU branch on MI355X: pcp_centerhead_targets_ext,
pcp_centerhead_loss_ext, HeadTrain over six heads and CenterHead.train() against the reference's own head (fixture g21,
tests/golden/make_golden_nusc_train.py) and the float64 statements of tests/nusc_head_refs.py."""
import json

import numpy as np
import pytest
import torch

import nusc_head_refs as refs
from helpers import load_golden
from pcp_amd import synth
from test_nusc_head_train_cpu import channels_of, geom_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LD = 16


@pytest.fixture(scope='module')
def g21():
    g = load_golden('g21_nusc_head_train.npz')
    g.update(load_golden('g21_nusc_head_train_grads.npz'))
    return g


def _target_desc(geom, B, K):
    from pcp_amd import lib
    return lib.Target(B, geom['h'], geom['w'], 0, K, geom['stride'], geom['voxel_x'], geom['voxel_y'], geom['min_x'], geom['min_y'],
                      geom['overlap'], geom['min_radius'])


def _padded(maps):
    buf = torch.zeros(maps.shape[:3] + (LD,))
    buf[..., :maps.shape[3]] = torch.from_numpy(maps)
    return buf.to(DEV)


def _fixture_heads(g):
    meta = g['meta']
    tables = refs.class_tables(meta['class_names'], meta['dense_head']['CLASS_NAMES_EACH_HEAD'])
    heads = []
    for hi in range(meta['n_heads']):
        off, reg, ncls = channels_of(meta, hi)
        heads.append(dict(num_class=ncls, class_to_local=tables[hi], head=_padded(g['h%d_maps' % hi]), ch_center=off['center'],
                          ch_z=off['center_z'], ch_dim=off['dim'], ch_rot=off['rot'], off=off, reg=reg))
    return heads


def _check_targets(got, want, iou_tol=None):
    for hi, ((heat, tb, inds, mask), w) in enumerate(zip(got, want)):
        assert np.array_equal(inds.cpu().numpy(), w['inds']) and np.array_equal(mask.cpu().numpy(), w['mask']), hi
        h = heat.cpu().numpy()
        assert np.array_equal(h == 1.0, w['heat'] == 1.0), hi
        np.testing.assert_allclose(h, w['heat'], rtol=0, atol=1e-6)
        t = tb.cpu().numpy()
        assert t.shape == w['tb'].shape, (hi, t.shape, w['tb'].shape)
        n = t.shape[-1] - (1 if iou_tol is not None else 0)
        np.testing.assert_allclose(t[..., :n], w['tb'][..., :n], rtol=0, atol=2e-6)
        if iou_tol is not None:
            err = np.abs(t[..., n] - w['tb'][..., n]).max()
            print('head %d: IoU target max err %.3e (bound %.3e)' % (hi, err, iou_tol))
            assert err <= iou_tol, (hi, err, iou_tol)


def test_targets_match_the_reference_fixture(g21):
    from pcp_amd import train_ops as tops
    g = g21
    meta = g['meta']
    geom = geom_of(meta, 32)
    gt = torch.from_numpy(g['gt_boxes']).to(DEV)
    got = tops.centerhead_targets_ext(gt, _target_desc(geom, 3, 500), _fixture_heads(g), with_iou=True)
    want = [dict(heat=g['h%d_heat' % h], tb=g['h%d_tb' % h], inds=g['h%d_inds' % h], mask=g['h%d_mask' % h]) for h in range(6)]
    _check_targets(got, want, iou_tol=max(2e-6, 4 * float(g['iou_f32_gap'])))
    assert gt.cpu().numpy().tobytes() == g['gt_boxes'].tobytes()                    # gt_boxes is only read


@pytest.mark.parametrize('width,M,K', [(8, 20, 8), (10, 20, 8), (10, 1, 8), (8, 300, 500)])
def test_targets_rank_cut_single_row_and_several_chunks_against_numpy(width, M, K):
    """K = 8 with more than 8 boxes of one head; M = 1; M = 300 (more rows than the 256 threads of a block: the rank carries over).
    The reference here is float64, the kernel float32 like the reference code: on an 8 x 8 map a centre coordinate is below 8 cells, so the
    three float32 roundings of (x - min) / voxel / stride stay below 3 * 2^-24 * 8 = 1.4e-6, inside the 2e-6 bound of the target boxes."""
    from pcp_amd import train_ops as tops
    names = ['car', 'truck', 'bus']
    tables = refs.class_tables(names, [['car'], ['truck', 'bus']])
    geom = dict(h=8, w=8, stride=4.0, voxel_x=float(np.float32(0.2)), voxel_y=float(np.float32(0.2)), min_x=-3.2, min_y=-3.2, overlap=0.1,
                min_radius=2)
    B = 2
    n = B * M
    s = 9100 + M + width
    gt = np.zeros((B, M, width), dtype=np.float32)
    gt[..., 0] = synth.uniform(s, 1, n, -3.6, 3.6).reshape(B, M)
    gt[..., 1] = synth.uniform(s, 2, n, -3.6, 3.6).reshape(B, M)
    gt[..., 2] = synth.uniform(s, 3, n, -3.0, 1.0).reshape(B, M)
    gt[..., 3:6] = synth.uniform(s, 4, 3 * n, 0.5, 4.0).reshape(B, M, 3)
    gt[..., 6] = synth.uniform(s, 5, n, -3.14159, 3.14159).reshape(B, M)
    if width == 10:
        gt[..., 7:9] = synth.uniform(s, 6, 2 * n, -3.0, 3.0).reshape(B, M, 2)
    cls = np.floor(synth.uniform(s, 7, n, 0.0, 3.999)).reshape(B, M)
    if M == 20:
        cls[0, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13]] = 1                             # 11 cars, rows of the other head in between
    if M == 1:
        cls[0, 0] = 3
    gt[..., -1] = cls
    frac = lambda c: np.abs(c - np.round(c))
    cx, cy = (gt[..., 0].astype(np.float64) + 3.2) / 0.8, (gt[..., 1].astype(np.float64) + 3.2) / 0.8
    gt[..., -1] = np.where((frac(cx) < 1e-3) | (frac(cy) < 1e-3), 0, gt[..., -1])    # float32 / float64 truncation must agree
    want = refs.assign_targets(gt, tables, geom, K)
    if M == 20:
        assert (gt[0, :, -1] == 1).sum() > K and want[0]['mask'][0].sum() == K       # the cut is exercised
    dev_gt = torch.from_numpy(gt).to(DEV)
    heads = [dict(num_class=max(t), class_to_local=t) for t in tables]
    got = tops.centerhead_targets_ext(dev_gt, _target_desc(geom, B, K), heads, with_iou=False)
    _check_targets(got, want)
    assert dev_gt.cpu().numpy().tobytes() == gt.tobytes()


def _loss_desc(meta, B, hw, K=500):
    from pcp_amd import lib
    lw = meta['dense_head']['LOSS_CONFIG']['LOSS_WEIGHTS']
    d = lib.HeadLossExt()
    d.batch, d.h, d.w, d.k = B, hw, hw, K
    d.cls_weight, d.loc_weight = float(lw['cls_weight']), float(lw['loc_weight'])
    for j, v in enumerate(lw['code_weights']):
        d.code_weights[j] = float(v)
    return d


def test_loss_and_gradient_match_the_reference_fixture(g21):
    from pcp_amd import train_ops as tops
    g = g21
    meta = g['meta']
    tb_ref = json.loads(str(g['tb_json']))
    heads = []
    for hi, h in enumerate(_fixture_heads(g)):
        heads.append(dict(head=h['head'], heat=torch.from_numpy(g['h%d_heat' % hi]).to(DEV), tb=torch.from_numpy(g['h%d_tb' % hi]).to(DEV),
                          inds=torch.from_numpy(g['h%d_inds' % hi]).to(DEV), mask=torch.from_numpy(g['h%d_mask' % hi]).to(DEV),
                          ch_hm=h['off']['hm'], num_class=h['num_class'], reg_ch=h['reg']))
    runs = [tops.centerhead_loss_ext(_loss_desc(meta, 3, 32), heads) for _ in range(2)]
    losses, total, dheads = runs[0]
    lv = losses.cpu().numpy()
    for hi in range(6):
        for col, key in ((0, 'hm_loss_head_%d' % hi), (1, 'loc_loss_head_%d' % hi)):
            print('%s: %.7g (reference %.7g)' % (key, lv[hi, col], tb_ref[key]))
            assert abs(lv[hi, col] - tb_ref[key]) <= 2e-5 * max(abs(tb_ref[key]), 1e-3), (key, lv[hi, col], tb_ref[key])
        want_sum = tb_ref['hm_loss_head_%d' % hi] + tb_ref['loc_loss_head_%d' % hi]
        assert abs(lv[hi, 2] - want_sum) <= 2e-5 * want_sum
        assert lv[hi, 3] == float((g['h%d_heat' % hi] == 1).sum())
        ref = g['h%d_dmaps' % hi].astype(np.float64)
        got = dheads[hi].cpu().numpy().astype(np.float64)
        nch = ref.shape[-1]
        assert np.abs(got[..., nch:]).max() == 0.0
        err = np.abs(got[..., :nch] - ref).max()
        assert err <= 2e-4 * max(np.abs(ref).max(), 1e-6), (hi, err, np.abs(ref).max())
    assert abs(float(total) - tb_ref['rpn_loss']) <= 2e-5 * abs(tb_ref['rpn_loss']), (float(total), tb_ref['rpn_loss'])
    # the same call again: the same bits (fixed-order float64 partials, slot-ordered gradient of boxes that share a cell)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


def test_loss_of_heads_without_positives_against_numpy(g21):
    """frame 0 alone: the barrier head has no box (num_pos = 0: the loss is -neg_loss, loss_utils.py:295-298; the L1 divisor clamps to 1)"""
    from pcp_amd import train_ops as tops
    g = g21
    meta = g['meta']
    lw = meta['dense_head']['LOSS_CONFIG']['LOSS_WEIGHTS']
    heads, want = [], []
    for hi, h in enumerate(_fixture_heads(g)):
        sl = lambda a: np.ascontiguousarray(a[:1])
        heads.append(dict(head=h['head'][:1].contiguous(), heat=torch.from_numpy(sl(g['h%d_heat' % hi])).to(DEV),
                          tb=torch.from_numpy(sl(g['h%d_tb' % hi])).to(DEV), inds=torch.from_numpy(sl(g['h%d_inds' % hi])).to(DEV),
                          mask=torch.from_numpy(sl(g['h%d_mask' % hi])).to(DEV), ch_hm=h['off']['hm'], num_class=h['num_class'],
                          reg_ch=h['reg']))
        want.append(refs.head_loss(sl(g['h%d_maps' % hi]), h['off']['hm'], h['num_class'], h['reg'], sl(g['h%d_heat' % hi]),
                                   sl(g['h%d_tb' % hi]).astype(np.float64), sl(g['h%d_inds' % hi]), sl(g['h%d_mask' % hi]),
                                   lw['code_weights'], lw['cls_weight'], lw['loc_weight']))
    assert want[3]['num_pos'] == 0 and want[3]['loc'] == 0.0 and want[3]['hm'] > 0
    losses, total, dheads = tops.centerhead_loss_ext(_loss_desc(meta, 1, 32), heads)
    lv = losses.cpu().numpy()
    for hi, w in enumerate(want):
        assert abs(lv[hi, 0] - w['hm']) <= 2e-5 * max(abs(w['hm']), 1e-3) and abs(lv[hi, 1] - w['loc']) <= 2e-5 * max(abs(w['loc']), 1e-3)
        assert lv[hi, 3] == w['num_pos']
        got = dheads[hi].cpu().numpy().astype(np.float64)
        nch = w['dmaps'].shape[-1]
        assert np.abs(got[..., nch:]).max() == 0.0
        assert np.abs(got[..., :nch] - w['dmaps']).max() <= 2e-4 * max(np.abs(w['dmaps']).max(), 1e-6), hi
    assert abs(float(total) - sum(w['hm'] + w['loc'] for w in want)) <= 2e-5 * float(total)


def _build_head(meta, dense_head=None, class_names=None):
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads.center_head import CenterHead
    class_names = class_names or meta['class_names']
    head = CenterHead(EasyDict(dense_head or meta['dense_head']), meta['input_channels'], len(class_names), class_names,
                      np.array(meta['grid_size']), np.array(meta['pc_range'], dtype=np.float32), meta['voxel_size'],
                      predict_boxes_when_training=False)
    shapes = {k: [int(x) for x in v.shape] for k, v in head.state_dict().items()}
    filled = synth.fill_state_dict(shapes, scheme=meta['scheme'])
    head.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return head.to(DEV).train(), shapes


def _feature(meta):
    f = meta['feature']
    return torch.from_numpy(synth.uniform(f['seed'], f['stream'], int(np.prod(f['shape'])), f['lo'], f['hi']).reshape(f['shape'])).to(DEV)


def _train_step(head, feat, gt):
    head.zero_grad()
    head({'spatial_features_2d': feat, 'gt_boxes': gt.clone(), 'batch_size': feat.shape[0]})
    loss, tb = head.get_loss()
    dx = head._backward_from_loss(None)
    return loss, tb, dx.t


def _sample(t, cap=4096):
    a = t.detach().reshape(-1)
    if a.numel() <= cap:
        return a.cpu().numpy()
    return a[::a.numel() // 1024][:1024].cpu().numpy()


@pytest.fixture(scope='module')
def head_step(g21):
    """one fp32 training step of CenterHead on the fixture's feature, shared by the tests below"""
    meta = g21['meta']
    head, shapes = _build_head(meta)
    feat = _feature(meta)
    gt = torch.from_numpy(g21['gt_boxes']).to(DEV)
    loss, tb, dx = _train_step(head, feat, gt)
    grads = {n: p.grad.clone() for n, p in head.named_parameters()}
    return dict(head=head, shapes=shapes, feat=feat, gt=gt, loss=loss, tb=tb, dx=dx, grads=grads)


def test_centerhead_train_mode_losses_and_dicts_match_the_reference_head(g21, head_step):
    g, meta, head, feat = g21, g21['meta'], head_step['head'], head_step['feat']
    assert head_step['shapes'] == meta['state_shapes']
    digest = g['feat_digest']
    assert abs(float(feat.double().sum()) - digest[0]) <= 1e-9 * abs(digest[0]) and float(feat.abs().max()) == digest[1]
    tb, loss = head_step['tb'], head_step['loss']
    tb_ref = json.loads(str(g['tb_json']))
    assert set(tb) == set(tb_ref) == {'rpn_loss'} | {'%s_loss_head_%d' % (k, i) for k in ('hm', 'loc') for i in range(6)}
    for k, v in tb_ref.items():
        print('%s: %.7g (reference %.7g)' % (k, tb[k], v))
        assert abs(tb[k] - v) <= 2e-4 * abs(v) + 1e-9, (k, tb[k], v)
    assert abs(float(loss) - float(g['loss'])) <= 2e-5 * float(g['loss']), (float(loss), float(g['loss']))
    td = head.forward_ret_dict['target_dicts']
    assert [len(td[k]) for k in ('heatmaps', 'target_boxes', 'inds', 'masks')] == [6] * 4 and len(head.forward_ret_dict['pred_dicts']) == 6
    for hi in range(6):
        assert np.array_equal(td['inds'][hi].cpu().numpy(), g['h%d_inds' % hi]) and td['target_boxes'][hi].shape == (3, 500, 11)
        assert td['heatmaps'][hi].shape == (3, g['h%d_heat' % hi].shape[-1], 32, 32)
        assert set(head.forward_ret_dict['pred_dicts'][hi]) == set(meta['branch_names'][hi])


def test_centerhead_train_mode_gradients_match_autograd(g21, head_step):
    """the bands test_single_model_train_step_matches_reference holds the head to: 3e-2 of the tensor's scale per tensor, 2e-2 global
    relative L2 over the sampled values"""
    g = g21
    names = [str(n) for n in g['param_names']]
    grads = head_step['grads']
    assert set(names) == set(n for n, p in head_step['head'].named_parameters() if p.requires_grad)
    gmax = max(float(np.abs(g['g/' + n]).max()) for n in names)
    num = den = 0.0
    for n in names:
        ref = g['g/' + n]
        mine = _sample(grads[n])
        scale = max(float(np.abs(ref).max()), 1e-4 * gmax)
        assert np.abs(mine - ref).max() <= 3e-2 * scale, (n, float(np.abs(mine - ref).max()), scale)
        num += float(((mine.astype(np.float64) - ref) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
    assert num <= (2e-2 ** 2) * den, (num / den) ** 0.5
    ref = g['dfeat_probe']
    mine = head_step['dx'].float().permute(0, 3, 1, 2)[:, ::16, ::2, ::2].cpu().numpy()
    assert np.abs(mine - ref).max() <= 3e-2 * np.abs(ref).max(), (np.abs(mine - ref).max(), np.abs(ref).max())
    rel = np.sqrt(((mine.astype(np.float64) - ref) ** 2).sum() / (ref.astype(np.float64) ** 2).sum())
    print('input-feature gradient: relative L2 %.3e; parameters %.3e' % (rel, (num / den) ** 0.5))
    assert rel <= 2e-2


def test_centerhead_train_step_repeats_bit_for_bit(head_step):
    loss2, _tb2, dx2 = _train_step(head_step['head'], head_step['feat'], head_step['gt'])
    assert torch.equal(head_step['loss'], loss2) and torch.equal(head_step['dx'], dx2)
    assert not [n for n, p in head_step['head'].named_parameters() if not torch.equal(p.grad, head_step['grads'][n])]


def test_centerhead_bf16_loop_step_tracks_the_fp32_loss(g21, head_step, monkeypatch):
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    head16, _ = _build_head(g21['meta'])
    loss16, _tb16, dx16 = _train_step(head16, head_step['feat'], head_step['gt'])
    loss = float(head_step['loss'])
    print('bf16 loop loss %.6f, fp32 %.6f' % (float(loss16), loss))
    assert dx16.dtype == torch.bfloat16 and abs(float(loss16) - loss) <= 1e-2 * loss
    assert all(torch.isfinite(p.grad).all() for p in head16.parameters()) and torch.isfinite(dx16.float()).all()


def test_loss_without_gradient_buffers_gives_the_same_losses(g21):
    """dhead NULL for every head: the two gradient launches are skipped, the losses are the same bits"""
    from pcp_amd import train_ops as tops
    g = g21
    heads = []
    for hi, h in enumerate(_fixture_heads(g)):
        heads.append(dict(head=h['head'], heat=torch.from_numpy(g['h%d_heat' % hi]).to(DEV), tb=torch.from_numpy(g['h%d_tb' % hi]).to(DEV),
                          inds=torch.from_numpy(g['h%d_inds' % hi]).to(DEV), mask=torch.from_numpy(g['h%d_mask' % hi]).to(DEV),
                          ch_hm=h['off']['hm'], num_class=h['num_class'], reg_ch=h['reg']))
    l1, t1, d1 = tops.centerhead_loss_ext(_loss_desc(g['meta'], 3, 32), heads, with_grad=True)
    l0, t0, d0 = tops.centerhead_loss_ext(_loss_desc(g['meta'], 3, 32), heads, with_grad=False)
    assert d0 is None and len(d1) == 6 and torch.equal(l0, l1) and torch.equal(t0, t1)


def test_predict_boxes_when_training_and_aliasing_layouts_stay_refused(g21):
    meta = g21['meta']
    head, _ = _build_head(meta)
    head.predict_boxes_when_training = True
    with pytest.raises(NotImplementedError, match='predict_boxes_when_training'):
        head({'spatial_features_2d': _feature(meta), 'gt_boxes': torch.from_numpy(g21['gt_boxes']).to(DEV), 'batch_size': 3})
    dh = json.loads(json.dumps(meta['dense_head']))
    dh['CLASS_NAMES_EACH_HEAD'] = [dh['CLASS_NAMES_EACH_HEAD'][1], dh['CLASS_NAMES_EACH_HEAD'][0]] + dh['CLASS_NAMES_EACH_HEAD'][2:]
    head, _ = _build_head(dict(meta, scheme='survey'), dense_head=dh)
    with pytest.raises(NotImplementedError, match='rewrites the class column'):
        head({'spatial_features_2d': _feature(meta), 'gt_boxes': torch.from_numpy(g21['gt_boxes']).to(DEV), 'batch_size': 3})


def test_one_head_eight_code_step_stays_on_the_old_entry_points(g21, monkeypatch):
    """the five V2X-Sim configs: one head, 8 codes, 8-column boxes -> pcp_centerhead_targets / pcp_centerhead_loss, never the _ext ones"""
    from pcp_amd import train_ops as tops
    meta = g21['meta']
    dh = json.loads(json.dumps(meta['dense_head']))
    dh['CLASS_NAMES_EACH_HEAD'] = [['car']]
    dh['SEPARATE_HEAD_CFG']['HEAD_ORDER'] = ['center', 'center_z', 'dim', 'rot']
    dh['SEPARATE_HEAD_CFG']['HEAD_DICT'] = {k: v for k, v in dh['SEPARATE_HEAD_CFG']['HEAD_DICT'].items() if k not in ('vel', 'iou')}
    dh['LOSS_CONFIG']['LOSS_WEIGHTS']['code_weights'] = [1.0] * 8
    head, _ = _build_head(meta, dense_head=dh, class_names=['car'])
    calls = []
    for name in ('centerhead_targets', 'centerhead_loss'):
        orig = getattr(tops, name)
        monkeypatch.setattr(tops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])

    def refuse(*a, **k):
        raise AssertionError('the one-head path must not reach the _ext entry points')
    monkeypatch.setattr(tops, 'centerhead_targets_ext', refuse)
    monkeypatch.setattr(tops, 'centerhead_loss_ext', refuse)
    gt = np.ascontiguousarray(np.concatenate([g21['gt_boxes'][..., :7], (g21['gt_boxes'][..., 9:] == 1).astype(np.float32)], -1))
    loss, tb, dx = _train_step(head, _feature(meta), torch.from_numpy(gt).to(DEV))
    assert calls == ['centerhead_targets', 'centerhead_loss'] and set(tb) == {'hm_loss_head_0', 'loc_loss_head_0', 'rpn_loss'}
    assert np.isfinite(float(loss)) and torch.isfinite(dx).all()


# ---- model level: CenterPoint on the V2X-Sim trunk (VFE, scatter, BaseBEVBackbone) with the six-head nuScenes DENSE_HEAD -----------------

@pytest.fixture(scope='module')
def g21m():
    g = load_golden('g21_nusc_model_train.npz')
    g.update(load_golden('g21_nusc_model_train_params.npz'))
    return g


def _model_and_optimizer(g):
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, 'practical-collab-perception_amd', 'tools'))
    from train_utils.optimization import build_optimizer, build_scheduler
    from pcdet.config import EasyDict
    from pcdet.models import build_network_from_meta
    meta = g['meta']
    model = build_network_from_meta(meta)
    st = synth.fill_state_dict(meta['state_shapes'])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(DEV)
    ocfg = EasyDict(meta['optimization'])
    opt = build_optimizer(model, ocfg)
    sched, _ = build_scheduler(opt, meta['total_it_each_epoch'], ocfg.NUM_EPOCHS, -1, ocfg)
    return model, opt, sched, ocfg


def _model_batch(g):
    return {'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}],
            'gt_boxes': torch.from_numpy(g['gt_boxes']).to(DEV)}


def _sample_cap(t, cap):
    a = t.detach().reshape(-1)
    if a.numel() <= cap:
        return a.cpu().numpy()
    return a[::a.numel() // 1024][:1024].cpu().numpy()


def test_model_train_steps_match_the_reference(g21m):
    """two iterations of the reference's train loop (fixture g21_nusc_model_train), structure and tolerances of
    test_gpu_train_e2e.py::test_single_model_train_step_matches_reference"""
    g = g21m
    meta = g['meta']
    cap = meta['sample_cap']
    names = [str(n) for n in g['trainable']]
    model, opt, sched, ocfg = _model_and_optimizer(g)
    params = dict(model.named_parameters())
    assert set(names) == set(n for n, p in params.items() if p.requires_grad)
    for it in range(2):
        sched.step(it)
        assert abs(opt.lr - float(g['it%d_lr' % it])) < 1e-12 and abs(opt.mom - float(g['it%d_mom' % it])) < 1e-12
        model.train()
        opt.zero_grad()
        batch = _model_batch(g)
        ret, tb, _disp = model(batch)
        loss = ret['loss']
        model.update_global_step()
        loss.backward()
        ref_tb = json.loads(str(g['it%d_tb_json' % it]))
        tol = 2e-5 if it == 0 else 3e-3
        lv = float(loss.detach())
        print('it %d: loss %.7g (reference %.7g)' % (it, lv, float(g['it%d_loss' % it])))
        assert abs(lv - float(g['it%d_loss' % it])) <= tol * abs(float(g['it%d_loss' % it])), (it, lv, float(g['it%d_loss' % it]))
        assert set(ref_tb) <= set(tb) and {'hm_loss_head_5', 'loc_loss_head_5', 'rpn_loss'} <= set(ref_tb)
        for k, v in ref_tb.items():
            assert abs(tb[k] - v) <= max(tol, 2e-4) * abs(v) + 1e-9, (k, tb[k], v)
        if it == 0:
            np.testing.assert_allclose(batch['spatial_features_2d'].detach().cpu().numpy()[:, ::8], g['map_probe'], rtol=0, atol=1e-4)
            gmax = max(float(np.abs(g['g0/' + n]).max()) for n in names)
            num = den = 0.0
            for n in names:
                ref = g['g0/' + n]
                mine = _sample_cap(params[n].grad, cap)
                scale = max(float(np.abs(ref).max()), 1e-4 * gmax)
                assert np.abs(mine - ref).max() <= 3e-2 * scale, (n, float(np.abs(mine - ref).max()), scale)
                num += float(((mine.astype(np.float64) - ref) ** 2).sum())
                den += float((ref.astype(np.float64) ** 2).sum())
            print('sampled gradients: global relative L2 %.3e' % ((num / den) ** 0.5))
            assert num <= (2e-2 ** 2) * den, (num / den) ** 0.5
        opt.clip_grad_norm(ocfg.GRAD_NORM_CLIP)
        opt.step()
        if it == 0:
            assert abs(opt.grad_norm() - float(g['it0_grad_norm'])) <= 5e-4 * float(g['it0_grad_norm'])
            for n in names:
                assert np.abs(_sample_cap(params[n], cap) - g['p1/' + n]).max() <= 2.1 * opt.lr, n
            sd = model.state_dict()
            for i, k in enumerate(str(k) for k in g['bn_keys']):
                a = sd[k].double()
                d = np.array([float(a.norm()), float(a.sum()), float(a.abs().max())])
                np.testing.assert_allclose(d, g['it0_bn_digest'][i], rtol=2e-4, atol=1e-6, err_msg=k)


def _model_first_step(g):
    model, opt, sched, _ocfg = _model_and_optimizer(g)
    sched.step(0)
    model.train()
    opt.zero_grad()
    ret, _tb, _disp = model(_model_batch(g))
    model.update_global_step()
    ret['loss'].backward()
    return float(ret['loss'].detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.fixture(scope='module')
def model_fp32_step(g21m):
    return _model_first_step(g21m)


def test_model_train_step_repeats_bit_for_bit(g21m, model_fp32_step):
    la, ga = model_fp32_step
    lb, gb = _model_first_step(g21m)
    assert la == lb and set(ga) == set(gb)
    assert not [n for n in ga if not torch.equal(ga[n], gb[n])]


def test_model_bf16_loop_iteration_tracks_the_fp32_loss(g21m, model_fp32_step, monkeypatch):
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    l16, g16 = _model_first_step(g21m)
    l32 = model_fp32_step[0]
    print('bf16 loop loss %.6f, fp32 %.6f' % (l16, l32))
    assert np.isfinite(l16) and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert all(torch.isfinite(v).all() for v in g16.values())
