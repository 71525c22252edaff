"""The float64 references of tests/glue_refs.py against independent statements of the same operations: oracle/anchor.py (torch fp32, pinned
to the reference's own detector by g9 / g11), the reference's recorded outputs where a fixture holds them, direct torch float64
expressions and oracle/hunter_train.py.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_refs as gr
from helpers import load_golden


def _oracle_decode(cls_map, box_map, dir_map, head_cfg, grid_size, pc_range):
    """oracle/anchor.py::head_forward fed with GIVEN head maps (B, H, W, k): the three 1x1 convs become exact channel selections"""
    from oracle import anchor as oan
    maps = [torch.from_numpy(np.ascontiguousarray(m)).permute(0, 3, 1, 2) for m in (cls_map, box_map, dir_map) if m is not None]
    x = torch.cat(maps, dim=1).contiguous()
    eye = torch.eye(x.shape[1]).view(x.shape[1], x.shape[1], 1, 1)
    st, o = {}, 0
    for name, m in zip(('conv_cls', 'conv_box', 'conv_dir_cls'), maps):
        st['dense_head.%s.weight' % name] = eye[o:o + m.shape[1]].contiguous()
        st['dense_head.%s.bias' % name] = torch.zeros(m.shape[1])
        o += m.shape[1]
    return oan.head_forward(x, st, head_cfg, grid_size, pc_range)


def _head_cfg(n_sizes, bins, limit_offset):
    sizes = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
    cfg = {'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': limit_offset, 'NUM_DIR_BINS': bins,
           'ANCHOR_GENERATOR_CONFIG': [{'class_name': 'c%d' % i, 'anchor_sizes': [sizes[i]], 'anchor_rotations': [0, float(np.float32(np.pi / 2))],
                                        'anchor_bottom_heights': [-1.0 - 0.3 * i], 'align_center': False, 'feature_map_stride': 1}
                                       for i in range(n_sizes)]}
    if bins:
        cfg['USE_DIRECTION_CLASSIFIER'] = True
    return cfg


@pytest.mark.parametrize('seed,B,H,W,n_sizes,ncls,bins,lim', [(1, 3, 5, 7, 3, 3, 2, 0.0), (2, 1, 4, 4, 1, 1, 2, 0.0), (3, 2, 3, 5, 1, 3, 0, 0.0),
                                                             (4, 2, 6, 5, 2, 2, 2, 0.5)])
def test_anchor_decode_reference_against_the_oracle_on_seeded_maps(seed, B, H, W, n_sizes, ncls, bins, lim):
    """boxes at the tolerance the decode kernels are held to (atol 1e-5, rtol 1e-6: the oracle is float32), direction bin / label exact,
    score and `>=` mask as oracle/anchor.py::post_process forms them.  The rotation residuals are redrawn until no anchor sits within
    1e-4 of a period boundary (checked below), so the float32 floor of the oracle takes the period of the float64 one."""
    A = 2 * n_sizes
    d = gr.draw_anchor_case(seed, B, H, W, A, ncls, bins, ld=A * (ncls + 7 + bins) + 3, ch_cls=1, ch_box=2 + A * ncls,
                            ch_dir=3 + A * (ncls + 7), dir_limit_offset=lim)
    head = d['head']
    cut = lambda s, n: head[..., s:s + n] if n else None
    cls_o, boxes_o, anchors_o = _oracle_decode(cut(1, A * ncls), cut(2 + A * ncls, A * 7), cut(3 + A * (ncls + 7), A * bins),
                                               _head_cfg(n_sizes, bins, lim), [W, H, 1], [-4.0, -4.0, -3.0, 4.0, 4.0, 1.0])
    anchors = anchors_o.numpy()
    ref = gr.anchor_decode(head, anchors, A, ncls, bins, 1, 2 + A * ncls, 3 + A * (ncls + 7), dir_limit_offset=lim, score_thresh=0.5)
    if bins:
        x = (gr.f64(head[..., 2 + A * ncls:2 + A * (ncls + 7)].reshape(B, -1, 7)[..., 6]) + gr.f64(anchors[None, :, 6])
             - float(gr.DIR_OFFSET)) / float(gr.DIR_PERIOD) + lim
        assert np.array_equal(anchors[:, 6], d['anchors'][:, 6]) and (x[d['exact']] == lim).all()
        assert (np.abs(x - np.round(x))[~d['exact']] >= 1e-4).all()
    assert np.array_equal(ref['cls'], cls_o.numpy())
    np.testing.assert_allclose(ref['boxes'], boxes_o.numpy(), rtol=1e-6, atol=1e-5)
    sc, lab = torch.max(torch.sigmoid(cls_o), dim=-1)
    assert np.array_equal(ref['labels'], lab.numpy())
    np.testing.assert_allclose(ref['scores'], sc.numpy(), rtol=0, atol=1e-6)
    assert np.array_equal(ref['mask'], (sc >= 0.5).numpy())
    assert ref['mask'].reshape(-1)[d['plant']['zero']].all() and (ref['scores'].reshape(-1)[d['plant']['zero']] == 0.5).all()
    assert (ref['labels'].reshape(-1)[d['plant']['cls_tie']] == 0).all()
    if len(d['plant']['cls_tie_hi']):
        assert (ref['labels'].reshape(-1)[d['plant']['cls_tie_hi']] == 1).all()
    if bins:
        assert (ref['dir_bin'].reshape(-1)[d['plant']['dir_tie']] == 0).all()
        frac = ref['dir_bin'].mean()
        assert 0.3 < frac < 0.7, frac
        assert len(np.unique(np.floor(ref['floor_arg']))) >= 4          # several periods occur


def test_limit_period_against_the_oracle():
    from oracle import anchor as oan
    v = np.random.RandomState(0).uniform(-12, 12, 4000)
    for off in (0.0, 0.5):
        got = gr.limit_period(v, off, np.pi)
        want = oan.limit_period(torch.from_numpy(v), off, np.pi).numpy()
        assert np.array_equal(got, want)
        assert (got >= -off * np.pi - 1e-12).all() and (got < (1 - off) * np.pi + 1e-12).all()


def test_anchor_decode_reference_on_the_reference_head_maps_of_g11():
    """The head maps the reference's own AnchorHeadSingle produced (tests/golden/g11_anchor_train.npz: cls / box / dir maps of iteration 0,
    three anchor classes x two rotations) decoded by glue_refs against oracle/anchor.py.  No committed fixture records both the head maps
    and the decoded boxes of one forward (g9 holds the decoded side, g11 the maps, of different clouds), so the oracle, pinned to g9's
    decoded boxes by test_g9_anchor_head_pointpillar, is the link.  Anchors closer than 1e-4 to a period boundary may take another
    period in float32 and are compared modulo the period; they are few."""
    g = load_golden('g11_anchor_train.npz')
    cfg = g['meta']['model']['DENSE_HEAD']
    cls_o, boxes_o, anchors_o = _oracle_decode(g['cls_preds'], g['box_preds'], g['dir_cls_preds'], cfg, [128, 128, 1], g['meta']['pc_range'])
    anchors = g['anchors'].reshape(-1, 7)
    assert np.array_equal(anchors_o.numpy(), anchors)
    head = np.concatenate([g['cls_preds'], g['box_preds'], g['dir_cls_preds']], axis=-1)
    ref = gr.anchor_decode(head, anchors, 6, 3, 2, 0, 18, 60, dir_offset=np.float32(cfg['DIR_OFFSET']),
                           dir_limit_offset=cfg['DIR_LIMIT_OFFSET'], dir_period=np.float32(np.pi))
    np.testing.assert_allclose(ref['boxes'][..., :6], boxes_o.numpy()[..., :6], rtol=1e-6, atol=1e-5)
    near = np.abs(ref['floor_arg'] - np.round(ref['floor_arg'])) < 1e-4
    assert near.mean() < 0.01
    dth = ref['boxes'][..., 6] - boxes_o.numpy()[..., 6]
    assert np.abs(dth[~near]).max() <= 1e-5
    assert np.abs(dth[near] - np.round(dth[near] / np.pi) * np.pi).max(initial=0.0) <= 1e-5
    assert 0.05 < ref['dir_bin'].mean() < 0.95


def test_anchor_scores_and_labels_reference_on_the_recorded_detections_of_g9():
    """tests/golden/g9_anchor_agnostic.npz records the reference's class logits, decoded boxes and final detections: every final detection
    is one decoded box, and its recorded score / 1-based label are the reference's sigmoid-max of that anchor's logits, above the mask"""
    g = load_golden('g9_anchor_agnostic.npz')
    thr = g['meta']['model']['POST_PROCESSING']['SCORE_THRESH']
    cls = g['batch_cls_preds']
    for b in range(cls.shape[0]):
        lab = np.argmax(cls[b], axis=-1)
        sc = gr.sigmoid(cls[b].max(-1))
        fb, fs, fl = g['final_boxes_%d' % b], g['final_scores_%d' % b], g['final_labels_%d' % b]
        assert fb.shape[0] > 10
        for i in range(fb.shape[0]):
            hit = np.nonzero((g['batch_box_preds'][b] == fb[i]).all(1))[0]
            assert hit.size >= 1
            j = hit[np.argmin(np.abs(sc[hit] - fs[i]))]
            assert abs(sc[j] - fs[i]) <= 1e-6 and lab[j] + 1 == fl[i] and sc[j] >= thr


def test_keys_to_scores_round_trip():
    s = np.array([0.5, 0.9999999, 1e-4, 1.0], np.float32)
    keys = (s.view(np.uint32) + 1).view(np.int32)
    assert np.array_equal(gr.keys_to_scores(keys), s.astype(np.float64))
    assert np.isnan(gr.keys_to_scores(np.zeros(1, np.int32))[0])
    assert (np.diff(gr.keys_to_scores(np.sort(keys))) > 0).all()


@pytest.mark.parametrize('pixels,c,thresh', [(1, 40, 0.05), (5, 64, 0.05), (203, 100, 0.05), (203, 40, 0.0), (7, 64, 1e-3)])
def test_masked_smooth_l1_reference_against_torch_float64(pixels, c, thresh):
    fused, teacher, zero = gr.draw_masked_sl1_case(11 + pixels, pixels, c, c + 8, c + 4, thresh)
    got, mask = gr.masked_smooth_l1_rows(fused, teacher, c, thresh)
    f, t = torch.from_numpy(fused[:, :c]).double(), torch.from_numpy(teacher[:, :c]).double()
    m = torch.linalg.norm(t, dim=1) > float(np.float32(thresh))
    want = F.smooth_l1_loss(f[m], t[m], reduction='none').sum(dim=1).mean()
    assert np.array_equal(mask, m.numpy()) and np.array_equal(mask, ~zero)
    np.testing.assert_allclose(got, float(want), rtol=1e-12)
    # the builder's promises: no row between the two norm classes, differences of exactly 1, 0 and -1 present, both branches taken
    norm = np.sqrt((gr.f64(teacher[:, :c]) ** 2).sum(1))
    assert ((norm == 0) | (norm >= 2 * thresh)).all()
    d = fused[~zero, :c] - teacher[~zero, :c]
    assert (d == 1.0).any() and (d == 0.0).any() and (d == -1.0).any()
    assert (np.abs(d) > 1).any() and (np.abs(d) < 1).any()


def test_masked_smooth_l1_reference_of_an_empty_selection_is_nan():
    fused, teacher, zero = gr.draw_masked_sl1_case(3, 9, 40, 48, 44, 0.05, all_zero=True)
    got, mask = gr.masked_smooth_l1_rows(fused, teacher, 40, 0.05)
    assert not mask.any() and np.isnan(got)
    want = F.smooth_l1_loss(torch.zeros(0, 40), torch.zeros(0, 40), reduction='none').sum(dim=1).mean()
    assert torch.isnan(want)


@pytest.mark.parametrize('seed,B,M,S,n', [(1, 2, 3, 5, 700), (2, 3, 7, 11, 9000), (0, 0, 0, 0, 0)])
def test_hunter_meta_and_centroid_references_against_the_oracle(seed, B, M, S, n):
    from oracle import hunter_train as oht
    if n:
        pts = gr.draw_hunter_cloud(seed, B, M, S, n)
    else:
        pts, B, M, S = gr.hand_made_hunter_cloud()
    meta = gr.hunter_meta(pts, M, S)
    p = torch.from_numpy(pts)
    o = oht.build_meta(p[p[:, -1] > -1], M, S)
    for mine, theirs in (('fg_local', 'locals2fg'), ('local_key', 'locals_bis'), ('local_inst', 'inst2locals'), ('inst_key', 'instance_bi'),
                         ('inst_last', 'indices_locals_max_sweep'), ('inst_first', 'indices_locals_min_sweep')):
        assert np.array_equal(meta[mine], o[theirs].numpy()), mine
    centroid, centered = gr.local_centroids(pts, meta)
    fg = p[p[:, -1] > -1, 1:4].double()
    want = torch.zeros(centroid.shape, dtype=torch.float64).index_add_(0, o['locals2fg'], fg)
    want = want / torch.bincount(o['locals2fg']).double()[:, None]
    np.testing.assert_allclose(centroid, want.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(centered, (fg - want[o['locals2fg']]).numpy(), rtol=0, atol=1e-12)
    c = 4
    rng = np.random.RandomState(seed)
    lf0, gf = rng.randn(len(meta['local_key']), c).astype(np.float32), rng.randn(len(meta['inst_key']), c).astype(np.float32)
    cen = centroid.astype(np.float32)
    lf0_t, gf_t = torch.from_numpy(lf0).double().requires_grad_(), torch.from_numpy(gf).double().requires_grad_()
    cat_t = torch.cat((lf0_t, gf_t[o['inst2locals']], torch.from_numpy(cen).double(),
                       torch.from_numpy(cen).double()[o['indices_locals_max_sweep']][o['inst2locals']]), dim=1)
    cat = gr.object_cat(lf0, gf, cen, meta, c, 16)
    assert np.array_equal(cat[:, :2 * c + 6].astype(np.float64), cat_t.detach().numpy()) and not cat[:, 2 * c + 6:].any()
    dcat = rng.rand(cat.shape[0], 16).astype(np.float32) + 0.5
    (cat_t * torch.from_numpy(dcat[:, :2 * c + 6]).double()).sum().backward()
    dlf0, dgf = gr.object_cat_backward(dcat, meta, c)
    assert np.array_equal(dlf0.astype(np.float64), lf0_t.grad.numpy())
    np.testing.assert_allclose(dgf, gf_t.grad.numpy(), rtol=1e-14)


def test_hand_made_hunter_cloud_holds_the_cases_it_names():
    pts, B, M, S = gr.hand_made_hunter_cloud()
    meta = gr.hunter_meta(pts, M, S)
    span = meta['inst_last'] - meta['inst_first']
    assert (span == 0).any() and (span == S - 1).any()                            # one sweep only; every sweep
    assert (np.bincount(meta['fg_local']) == 1).any()                             # a local with a single point
    assert (pts[:, 0] == 1).any() and not (pts[pts[:, 0] == 1, -1] > -1).any()    # a frame without foreground
    assert (meta['inst_key'] // M == 0).all()


def test_small_references_on_hand_checked_cases():
    head = np.array([[1, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [1, 1, 1, 0, 0, 0], [-3, -3, -2, 0, 0, 0], [0, 0, 2, 0, 0, 0]], np.float32)
    mask, p2 = gr.apply_flow_mask(head, 0.3)
    assert mask.tolist() == [False, False, False, False, True] and abs(p2[3] - 1 / (1 + np.exp(2.0))) < 1e-15
    pts = np.zeros((6, 3), np.float32)
    pts[:, 0] = [0, 1, -1, 2, 0, 1]
    pts[:, 2] = [3, 3, 4, 5, -1, 63]
    live = gr.agent_frame_live(pts, 2, 2).reshape(64, 2)
    assert live.sum() == 4 and live[3].tolist() == [1, 1] and live[63].tolist() == [1, 1] and not live[4].any() and not live[5].any()
    assert not gr.agent_frame_live(np.zeros((0, 3), np.float32), 2, 3).any()
    maps = np.arange(12, dtype=np.float32).reshape(3, 4) - 5
    out = gr.zero_maps_unless(maps, [-1, 0, 1], np.array([0, 1], np.int32))
    assert np.array_equal(out[0], maps[0]) and not out[1].any() and np.array_equal(out[2], maps[2])
    dst = np.ones((5, 6), np.float32)
    out = gr.rows_scatter_add(np.full((2, 4), 2, np.float32), [1, 3], 3, dst)
    assert out.sum() == 30 + 12 and out[1, :3].tolist() == [3, 3, 3] and out[1, 3] == 1 and (out[[0, 2, 4]] == 1).all()
