"""Operator-level tests of the small elementwise / segment kernels that otherwise run only inside whole-model fixtures, each against the
plain float64 reference of tests/glue_refs.py (checked on the CPU by tests/test_glue_refs_cpu.py) at the shapes and planted inputs where
such a kernel can be wrong: ties, `>` against `>=`, thread counts that are no multiple of the block, strides wider than the payload with
garbage in the padding, empty and out-of-range rows.  Integer outputs, gathers and single float32 additions are compared bit for bit;
float tolerances are derived per test.  GPU only."""
import numpy as np
import pytest
import torch

import glue_refs as gr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS = 2.0 ** -24          # half a float32 ulp, relative


def _bits(x):
    """int32 view of a float32 array / tensor on the host: equality of these is equality bit for bit (-0.0 != +0.0, nan payloads kept)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# pcp_anchor_decode
# ---------------------------------------------------------------------------------------------------------------------
# name: (seed, B, H, W, A, classes, dir bins, ld, ch_cls, ch_box, ch_dir, dir_limit_offset)
#   odd630    3 * 5 * 7 * 6 = 630 threads (2.46 blocks); the three channel groups start past 0 and are separated by garbage channels.
#             6 anchors x (3 + 7 + 2) channels are 72, so the row is 80 wide (64 cannot hold the groups)
#   single    one class, the head's own packed layout
#   nodir     no direction classifier: the rotation is residual + anchor, no period arithmetic
#   blocks    1024 threads: four full blocks
#   limit05   dir_limit_offset 0.5: the period is taken around val instead of above it
ANCHOR_CASES = {
    'odd630': (1, 3, 5, 7, 6, 3, 2, 80, 1, 21, 65, 0.0),
    'single': (2, 1, 4, 4, 2, 1, 2, 20, 0, 2, 16, 0.0),
    'nodir': (3, 2, 3, 5, 2, 3, 0, 24, 2, 9, 0, 0.0),
    'blocks': (4, 2, 16, 16, 2, 2, 2, 24, 0, 4, 18, 0.0),
    'limit05': (5, 2, 6, 5, 4, 2, 2, 48, 1, 10, 39, 0.5),
}


def _anchor_desc(B, H, W, A, ncls, bins, ld, ch_cls, ch_box, ch_dir, lim, use_thresh):
    from pcp_amd import lib
    return lib.Anchor(B, H, W, ld, A, ncls, bins, ch_cls, ch_box, ch_dir, float(gr.DIR_OFFSET), float(np.float32(lim)), float(gr.DIR_PERIOD),
                      1 if use_thresh else 0, 0.5)


@pytest.mark.parametrize('name', sorted(ANCHOR_CASES))
def test_anchor_decode_against_the_float64_reference(name):
    """Boxes at atol 1e-5 / rtol 1e-6 (the tolerances of test_decode_ext_two_class_128 for the same arithmetic: a handful of float32
    roundings on values below 16), every anchor compared.  The inputs keep every anchor's floor argument 1e-4 away from an integer
    (asserted on the reference first), so the kernel's float32 floor cannot take another period; the planted anchors whose residual IS
    dir_offset (val = 0 exactly, in float32 and float64) must come out as dir_offset + period * bin bit for bit.  Planted ties go to the
    lower index (class label and direction bin), the class logits pass through bit for bit, and the score keys follow the `>= 0.5` mask
    exactly: a logit of exactly 0 is a score of exactly 0.5 and is kept, every other maximal logit is at least 1e-3 from 0."""
    from pcp_amd import ops
    seed, B, H, W, A, ncls, bins, ld, ch_cls, ch_box, ch_dir, lim = ANCHOR_CASES[name]
    d = gr.draw_anchor_case(seed, B, H, W, A, ncls, bins, ld, ch_cls, ch_box, ch_dir, dir_limit_offset=lim)
    head, anchors, exact, plant = d['head'], d['anchors'], d['exact'], d['plant']
    N = H * W * A
    ref = gr.anchor_decode(head, anchors, A, ncls, bins, ch_cls, ch_box, ch_dir, dir_limit_offset=np.float32(lim), score_thresh=0.5)
    # ---- the inputs hold what the test is about (reference only, before the kernel runs)
    assert set(np.unique(anchors[:, 6])) == {np.float32(0.0), np.float32(np.pi / 2)} and (anchors[:, 3] != anchors[:, 4]).all()
    mx = ref['cls'].max(-1)
    assert ((np.abs(mx) >= 1e-3) | (mx == 0)).all() and (mx.reshape(-1)[plant['zero']] == 0).all()
    assert (ref['scores'].reshape(-1)[plant['zero']] == 0.5).all() and ref['mask'].reshape(-1)[plant['zero']].all()
    assert ref['mask'].any() and not ref['mask'].all()
    if bins:
        x = ref['floor_arg']
        assert (np.abs(x - np.round(x))[~exact] >= 1e-4).all()
        assert exact.sum() >= 3 and (x[exact] == float(np.float32(lim))).all()
        e6 = head.reshape(B, H * W, ld)[:, :, ch_box:ch_box + 7 * A].reshape(B, N, 7)[..., 6]
        assert ((e6 + anchors[None, :, 6])[exact] == gr.DIR_OFFSET).all()                 # float32 sum: val is exactly 0 in the kernel too
        assert 0.3 < ref['dir_bin'].mean() < 0.7 and len(np.unique(np.floor(x))) >= 4     # both bins, several periods
    # ---- kernel
    hd, an = torch.from_numpy(head).to(DEV), torch.from_numpy(anchors).to(DEV)
    boxes, cls, keys, labels = ops.anchor_decode(hd, an, _anchor_desc(B, H, W, A, ncls, bins, ld, ch_cls, ch_box, ch_dir, lim, True))
    boxes, cls, keys, labels = boxes.cpu().numpy(), cls.cpu().numpy(), keys.cpu().numpy(), labels.cpu().numpy()
    err = np.abs(boxes - ref['boxes'])
    print('%s seed %d: max box err %.3g (angle %.3g)' % (name, d['seed'], err.max(), err[..., 6].max()))
    np.testing.assert_allclose(boxes, ref['boxes'], rtol=1e-6, atol=1e-5)
    if bins:
        want = (gr.DIR_OFFSET + gr.DIR_PERIOD * ref['dir_bin'][exact].astype(np.float32)).astype(np.float32)
        assert np.array_equal(_bits(boxes[..., 6][exact]), _bits(want))
        assert set(ref['dir_bin'][exact]) == {0, 1}
    assert np.array_equal(_bits(cls), _bits(ref['cls']))
    assert np.array_equal(labels, ref['labels'])
    assert (labels.reshape(-1)[plant['cls_tie']] == 0).all()
    if len(plant['cls_tie_hi']):
        assert (labels.reshape(-1)[plant['cls_tie_hi']] == 1).all()
    # ---- score keys
    k = keys.astype(np.int64) & 0xffffffff
    assert np.array_equal(k == 0, ~ref['mask'])
    assert (k.reshape(-1)[plant['zero']] == int(np.float32(0.5).view(np.uint32)) + 1).all()
    kept = ref['mask']
    sc = gr.keys_to_scores(keys)
    assert np.abs(sc[kept] - ref['scores'][kept]).max() <= 1e-6
    order = np.argsort(ref['scores'][kept], kind='stable')
    ks, rs = k[kept][order], ref['scores'][kept][order]
    assert ((np.diff(ks) >= 0) | (np.diff(rs) <= 2e-6)).all()                             # key order is score order
    # ---- no threshold: nothing is masked, everything else unchanged
    b2, c2, k2, l2 = ops.anchor_decode(hd, an, _anchor_desc(B, H, W, A, ncls, bins, ld, ch_cls, ch_box, ch_dir, lim, False))
    k2 = k2.cpu().numpy().astype(np.int64) & 0xffffffff
    assert (k2 != 0).all() and np.array_equal(k2[kept], k[kept])
    assert np.abs(gr.keys_to_scores(k2) - ref['scores']).max() <= 1e-6
    assert np.array_equal(_bits(b2), _bits(boxes)) and np.array_equal(l2.cpu().numpy(), labels)


# ---------------------------------------------------------------------------------------------------------------------
# pcp_hunter_apply_flow
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stride', [5, 11])
def test_hunter_apply_flow_mask_and_in_place_update(stride):
    """1000 rows (3.9 blocks), head rows 8 wide, threshold 0.3.  Every drawn row keeps l2 at least 1e-3 from both other logits and p2 at
    least 1e-3 from the threshold in float64, so the float32 comparisons of the kernel cannot differ from the float64 ones; ties are
    planted exactly (equal float32 logits give equal float32 sigmoids): class 2 equal to the best other class is NOT dynamic (torch.max
    returns the first maximal index), and class 2 as the clear maximum below the threshold is not either.  Dynamic rows get one float32
    addition per coordinate, everything else in `points` keeps its bits."""
    from pcp_amd import ops
    n, thresh = 1000, 0.3
    rng = np.random.RandomState(40 + stride)
    head = rng.uniform(-3.0, 3.0, (n, 8)).astype(np.float32)
    head[:, 3:6] = rng.randn(n, 3).astype(np.float32)
    head[:, 6:] = rng.uniform(-1e3, 1e3, (n, 2)).astype(np.float32)
    planted = {'l2 == l0 > l1': (1.0, 0.0, 1.0), 'l2 == l1 > l0': (-0.5, 0.75, 0.75), 'all equal': (0.5, 0.5, 0.5),
               'class 2 best, below the threshold': (-2.5, -3.0, -1.5), 'class 2 best, above': (-2.5, -3.0, -0.5)}
    rows = {}
    for i, (what, v) in enumerate(planted.items()):
        rows[what] = np.arange(7 + 13 * i, n, 97)[:8]
        head[rows[what], :3] = v
    free = np.ones(n, bool)
    free[np.concatenate(list(rows.values()))] = False
    for _ in range(100):
        p2 = gr.sigmoid(head[:, 2])
        bad = free & ((np.abs(head[:, 2] - head[:, 0]) < 1e-3) | (np.abs(head[:, 2] - head[:, 1]) < 1e-3) | (np.abs(p2 - np.float32(thresh)) < 1e-3))
        if not bad.any():
            break
        head[bad, :3] = rng.uniform(-3.0, 3.0, (int(bad.sum()), 3)).astype(np.float32)
    assert not bad.any()
    mask, p2 = gr.apply_flow_mask(head, thresh)
    assert (np.abs(p2 - float(np.float32(thresh))) >= 1e-3).all() and 0.15 < mask.mean() < 0.5
    for what, r in rows.items():
        assert mask[r].all() == (what == 'class 2 best, above') and mask[r].any() == (what == 'class 2 best, above'), what
    pts = rng.uniform(-60.0, 60.0, (n, stride)).astype(np.float32)
    pts[:, 0] = rng.randint(0, 4, n)
    pts[::17, 1:4] = -0.0
    want = pts.copy()
    moved = torch.from_numpy(pts[:, 1:4]) + torch.from_numpy(head[:, 3:6])                # torch float32 xyz + flow
    want[mask, 1:4] = moved.numpy()[mask]
    p = torch.from_numpy(pts).to(DEV)
    got_mask = ops.hunter_apply_flow(p, torch.from_numpy(head).to(DEV), thresh)
    assert got_mask.dtype == torch.uint8 and np.array_equal(got_mask.cpu().numpy(), mask.astype(np.uint8))
    assert np.array_equal(_bits(p), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# HunterJr object-head glue: pcp_hunter_local_centroids, pcp_hunter_object_cat, pcp_hunter_object_cat_backward, pcp_rows_scatter_add
# ---------------------------------------------------------------------------------------------------------------------

def _hunter_cloud(name):
    if name == 'hand':
        return gr.hand_made_hunter_cloud()
    seed, B, M, S, n = {'small': (1, 2, 3, 5, 700), 'large': (2, 3, 7, 11, 9000)}[name]
    return gr.draw_hunter_cloud(seed, B, M, S, n), B, M, S


_META_CACHE = {}


def _hunter_meta(name):
    """(points numpy, device points, device meta of pcp_hunter_meta, numpy reference meta); the device meta is checked against the
    reference once, so the tests below index with either"""
    if name not in _META_CACHE:
        from pcp_amd import train_ops as tops
        pts, B, M, S = _hunter_cloud(name)
        pd = torch.from_numpy(pts).to(DEV)
        m = tops.hunter_meta(pd, B, M, S, -2, -1)
        ref = gr.hunter_meta(pts, M, S)
        assert (m.n_fg, m.n_local, m.n_inst, m.bad_rows) == (len(ref['fg_idx']), len(ref['local_key']), len(ref['inst_key']), 0)
        for key, cnt in (('fg_idx', m.n_fg), ('fg_local', m.n_fg), ('local_key', m.n_local), ('local_inst', m.n_local), ('inst_key', m.n_inst),
                         ('inst_first', m.n_inst), ('inst_last', m.n_inst)):
            assert np.array_equal(getattr(m, key)[:cnt].cpu().numpy(), ref[key]), key
        _META_CACHE[name] = (pts, pd, m, ref, S)
    return _META_CACHE[name]


def _assert_hand_cases(name, ref, S):
    if name != 'hand':
        return
    span = ref['inst_last'] - ref['inst_first']
    assert (span == 0).any() and (span == S - 1).any() and (np.bincount(ref['fg_local']) == 1).any()


@pytest.mark.parametrize('name', ['small', 'large', 'hand'])
def test_hunter_local_centroids_against_float64_scatter_mean(name):
    """The kernel sums each local in float64 (atomics: the order does not reach float32), rounds the sum to float32 and divides by the
    float32 count: the sum's rounding and the division are 2 * 2**-24 relative to the centroid, allowed 4 * 2**-24 of the largest
    coordinate.  centered = one float32 subtraction of that centroid: 4 (centroid) + 2 (difference of two values below max) ulps halves,
    allowed 8 * 2**-24 * max|xyz|; the columns past xyz of the 16-wide rows are exactly +0."""
    from pcp_amd import train_ops as tops
    pts, pd, m, ref, S = _hunter_meta(name)
    _assert_hand_cases(name, ref, S)
    centroid, centered = tops.hunter_local_centroids(pd, m, 16)
    want_c, want_d = gr.local_centroids(pts, ref)
    big = float(np.abs(pts[:, 1:4]).max())
    centroid, centered = centroid.cpu().numpy(), centered.cpu().numpy()
    assert centroid.shape == want_c.shape and centered.shape == (m.n_fg, 16)
    e_c, e_d = np.abs(centroid - want_c).max(), np.abs(centered[:, :3] - want_d).max()
    print('%s: centroid err %.3g (bound %.3g), centered err %.3g (bound %.3g)' % (name, e_c, 4 * EPS * big, e_d, 8 * EPS * big))
    assert e_c <= 4 * EPS * big
    assert e_d <= 8 * EPS * big
    assert not _bits(centered[:, 3:]).any()
    single = np.bincount(ref['fg_local']) == 1                      # a local of one point is that point
    if single.any():
        first = np.array([np.nonzero(ref['fg_local'] == l)[0][0] for l in np.nonzero(single)[0]])
        assert np.array_equal(centroid[single], pts[ref['fg_idx'][first], 1:4])


@pytest.mark.parametrize('name,c', [('small', 32), ('large', 32), ('hand', 32), ('large', 24)])
def test_hunter_object_cat_is_the_gather_and_its_backward_the_segment_sum(name, c):
    """Forward: [lf0 | gf[inst] | centroid | centroid[last-sweep local of inst] | 0 ...] bit for bit, rows round_up(2c + 6, 16) wide.  The
    centroids are random rows, so the own centroid and the last-sweep local's centroid differ wherever an instance has two locals.
    Backward: dlf0 is the slice bit for bit; dgf sums the (all positive, so nothing cancels) gradients of at most S <= 11 locals in
    float32 in a fixed order: S * 2**-24 < 1e-6 relative to the float64 sum."""
    from pcp_amd import pack
    from pcp_amd import train_ops as tops
    pts, pd, m, ref, S = _hunter_meta(name)
    _assert_hand_cases(name, ref, S)
    ld = pack.round_up(2 * c + 6, 16)
    assert ld == {32: 80, 24: 64}[c] and S * EPS < 1e-6
    rng = np.random.RandomState(c + len(name))
    lf0, gf = rng.randn(m.n_local, c).astype(np.float32), rng.randn(m.n_inst, c).astype(np.float32)
    cen = rng.randn(m.n_local, 3).astype(np.float32)
    assert (ref['inst_last'][ref['local_inst']] != np.arange(m.n_local)).any()
    out = tops.hunter_object_cat(torch.from_numpy(lf0).to(DEV), torch.from_numpy(gf).to(DEV), torch.from_numpy(cen).to(DEV), m, c, ld)
    assert np.array_equal(_bits(out), _bits(gr.object_cat(lf0, gf, cen, ref, c, ld)))
    dcat = rng.uniform(0.5, 1.5, (m.n_local, ld)).astype(np.float32)
    dlf0, dgf = tops.hunter_object_cat_backward(torch.from_numpy(dcat).to(DEV), m, c)
    want_l, want_g = gr.object_cat_backward(dcat, ref, c)
    assert np.array_equal(_bits(dlf0), _bits(want_l))
    print('%s c=%d: dgf max rel err %.3g' % (name, c, np.abs(dgf.cpu().numpy() / want_g - 1).max()))
    np.testing.assert_allclose(dgf.cpu().numpy(), want_g, rtol=1e-6, atol=0)


def test_rows_scatter_add_touches_only_the_selected_windows():
    """37 rows x 32 channels = 1184 threads (4.6 blocks), source rows 40 wide, destination rows 48 wide, a sorted random subset of the
    destination rows: the selected 32-channel windows are dst + src in float32 bit for bit, everything else keeps its bits; zero rows
    (the entry point returns before the launch) change nothing."""
    from pcp_amd import train_ops as tops
    rng = np.random.RandomState(9)
    rows, c, n = 37, 32, 120
    assert (rows * c) % 256 != 0
    src = rng.randn(rows, 40).astype(np.float32)
    dst = rng.randn(n, 48).astype(np.float32)
    idx = np.sort(rng.permutation(n)[:rows]).astype(np.int32)
    want = gr.rows_scatter_add(src, idx, c, dst)
    d = torch.from_numpy(dst).to(DEV)
    tops.rows_scatter_add(torch.from_numpy(src).to(DEV), torch.from_numpy(idx).to(DEV), 0, c, d)
    assert np.array_equal(_bits(d), _bits(dst))
    tops.rows_scatter_add(torch.from_numpy(src).to(DEV), torch.from_numpy(idx).to(DEV), rows, c, d)
    assert np.array_equal(_bits(d), _bits(want))
    untouched = np.ones((n, 48), bool)
    untouched[idx, :c] = False
    assert np.array_equal(_bits(d)[untouched], _bits(dst)[untouched]) and (_bits(d)[~untouched] != _bits(dst)[~untouched]).mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------------
# pcp_masked_smooth_l1_rows
# ---------------------------------------------------------------------------------------------------------------------
MSL_THRESH = 0.05


def _msl(fused, teacher, c, thresh):
    from pcp_amd import train_ops as tops
    f = torch.from_numpy(fused).to(DEV).view(1, 1, fused.shape[0], fused.shape[1])
    t = torch.from_numpy(teacher).to(DEV).view(1, 1, teacher.shape[0], teacher.shape[1])
    return tops.masked_smooth_l1_rows(f, t, c, thresh).cpu().numpy()


@pytest.mark.parametrize('c', [40, 64, 100])
@pytest.mark.parametrize('pixels', [1, 3, 4, 5, 5003])
def test_masked_smooth_l1_rows_against_float64(pixels, c):
    """One wavefront per pixel, four per block, at most 1024 blocks: 5003 pixels are past 4 x 1024, so the stride loop runs; 1..5 pixels
    leave waves of the last block idle.  Rows 8 (fused) and 4 (teacher) wider than c with garbage behind.  Teacher rows are exactly zero
    or have a norm of at least 2 * thresh, so the `> thresh` mask is exact; differences straddle |d| = 1 with exact 1, 0 and -1 planted.
    Error: per row ceil(c / 64) float32 additions per lane, 6 in the butterfly, 2 in the term itself, all terms positive:
    (ceil(c / 64) + 8) * 2**-24 <= 6e-7 relative, float64 from there, one rounding of the result; rtol 1e-5 leaves room."""
    fused, teacher, zero = gr.draw_masked_sl1_case(100 * c + pixels, pixels, c, c + 8, c + 4, MSL_THRESH)
    want, mask = gr.masked_smooth_l1_rows(fused, teacher, c, MSL_THRESH)
    assert np.array_equal(mask, ~zero) and mask.any() and (pixels < 3 or zero.any())
    assert ((-(-c // 64)) + 8) * EPS < 1e-5
    got = _msl(fused, teacher, c, MSL_THRESH)
    print('pixels %d c %d: %.9g vs %.9g, rel %.3g' % (pixels, c, got[0], want, abs(got[0] / want - 1)))
    np.testing.assert_allclose(got[0], want, rtol=1e-5, atol=0)
    assert np.array_equal(_bits(_msl(fused, teacher, c, MSL_THRESH)), _bits(got))         # fixed reduction order: same bits again


@pytest.mark.parametrize('pixels,c', [(5, 40), (5003, 100)])
def test_masked_smooth_l1_rows_threshold_zero_excludes_exactly_the_zero_rows(pixels, c):
    """thresh = 0: the mask is strict, a zero teacher row (norm 0) stays out and every other row, however small, is in"""
    fused, teacher, zero = gr.draw_masked_sl1_case(7 * c + pixels, pixels, c, c + 8, c + 4, 0.0)
    fused[zero, :c] += np.float32(3.0)                                                    # a zero row that got in would move the mean
    want, mask = gr.masked_smooth_l1_rows(fused, teacher, c, 0.0)
    with_zero_rows, _ = gr.masked_smooth_l1_rows(fused, teacher + np.float32(1e-30), c, 0.0)
    assert np.array_equal(mask, ~zero) and zero.any() and abs(with_zero_rows / want - 1) > 0.1
    np.testing.assert_allclose(_msl(fused, teacher, c, 0.0)[0], want, rtol=1e-5, atol=0)


@pytest.mark.parametrize('pixels,thresh', [(1, MSL_THRESH), (9, MSL_THRESH), (9, 0.0)])
def test_masked_smooth_l1_rows_of_an_empty_selection_is_nan(pixels, thresh):
    fused, teacher, zero = gr.draw_masked_sl1_case(5, pixels, 64, 72, 68, thresh, all_zero=True)
    assert zero.all() and np.isnan(gr.masked_smooth_l1_rows(fused, teacher, 64, thresh)[0])
    assert np.isnan(_msl(fused, teacher, 64, thresh)[0])


# ---------------------------------------------------------------------------------------------------------------------
# pcp_agent_frame_live, pcp_zero_maps_unless
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('batch', [1, 4, 64])
@pytest.mark.parametrize('n', [0, 10, 10000])
def test_agent_frame_live_flags_against_numpy(n, batch):
    """All 64 x batch flags.  Agent ids from {-1, 0, 1, 2, 63}; agent 3 holds one row in one frame only (live in EVERY frame: which
    frames exist is metadata), agent 4 only rows whose frame index is -1 or `batch` (ignored: no flag), agent 5 no row at all; agent 0
    also holds an out-of-range row.  10 000 rows are three blocks of the histogram kernel, 0 rows skip it."""
    from pcp_amd import ops
    rng = np.random.RandomState(1000 * batch + n)
    stride = 7
    pts = rng.randn(n, stride).astype(np.float32)
    if n:
        pts[:, 0] = rng.randint(0, batch, n)
        pts[:, -1] = np.array([-1, 0, 1, 2, 63], np.float32)[rng.randint(0, 5, n)]
        pts[:6, 0] = [batch - 1, -1, batch, -1, 0, batch - 1]
        pts[:6, -1] = [3, 4, 4, 0, 63, -1]
    want = gr.agent_frame_live(pts, stride - 1, batch)
    if n:
        w = want.reshape(64, batch)
        assert w[3].all() and not w[4].any() and not w[5].any() and w[63].all() and w[6:63].sum() == 0
    else:
        assert not want.any()
    live = ops.agent_frame_live(torch.from_numpy(pts).to(DEV), -1, batch)
    assert live.dtype == torch.int32 and np.array_equal(live.cpu().numpy(), want)


ZM_BIG = 512 * 256 * 8 * 4 + 4          # one float4 more than the largest grid covers in one pass


@pytest.mark.parametrize('elems', [4, 1028, ZM_BIG])
@pytest.mark.parametrize('n_maps', [1, 7])
def test_zero_maps_unless_zeroes_exactly_the_dead_maps(n_maps, elems):
    """Maps of one float4, of 257 float4 (two waves more than a block) and of one float4 more than 512 blocks x 256 threads x 8 cover
    (the stride loop).  Flag indices: -1 (never zeroed), a live flag, a dead flag.  Dead maps are +0.0 in every bit, live and -1 maps and
    the guard elements behind the last map keep their bits.  With one map the three kinds of index are tried in turn."""
    from pcp_amd import ops
    live_host = np.array([0, 1, 0, 7, 0, -3, 0, 0], np.int32)
    live = torch.from_numpy(live_host).to(DEV)
    tables = [[-1, 1, 0, 3, 2, -1, 5][:n_maps]] if n_maps > 1 else [[-1], [1], [2], [5], [4]]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(elems + n_maps)
    src = torch.randn(n_maps * elems + 4, device=DEV, generator=gen) - 0.25
    src[::3] = -0.0
    for idx in tables:
        buf = src.clone()
        maps = buf[:n_maps * elems].view(n_maps, elems)
        ops.zero_maps_unless(maps, idx, live)
        got, orig = buf.view(torch.int32), src.view(torch.int32)
        dead = [k >= 0 and live_host[k] == 0 for k in idx]
        assert any(dead) or n_maps == 1
        for m_i, is_dead in enumerate(dead):
            g = got[m_i * elems:(m_i + 1) * elems]
            if is_dead:
                assert not bool(g.any()), (idx, m_i)
            else:
                assert torch.equal(g, orig[m_i * elems:(m_i + 1) * elems]), (idx, m_i)
        assert torch.equal(got[n_maps * elems:], orig[n_maps * elems:])
        if elems <= 1028:                               # the numpy reference on the sizes worth a host copy
            want = gr.zero_maps_unless(src[:n_maps * elems].view(n_maps, elems).cpu().numpy(), idx, live_host)
            assert np.array_equal(_bits(maps), _bits(want))
