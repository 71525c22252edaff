"""csrc/nms.hip and csrc/bev_geom.h (k_pairwise, k_nms_sort, k_nms_identity, k_nms_mask, k_nms_greedy) through pcp_amd.ops against the float64
clipper and the structural cases of tests/bev_iou_refs.py: pairwise IoU / overlap against true rectangle geometry, the degenerate table against
closed forms, the production call shape (batched, ragged n_dev, scores=None, pre_max < n), sweep cases whose verdicts are far from the
threshold by construction, the sort against the reference's stable descending order, and the limits.
Run on the GPU box:  python -m pytest tests/test_gpu_bev_iou.py -m gpu -q
"""
import functools

import numpy as np
import pytest
import torch

import bev_iou_refs as R
from oracle import nms as onms

pytestmark = pytest.mark.gpu

THR = 0.2
GPU_VS_ORACLE = 2e-5        # sinf / cosf / atan2f differ by ulps between ocml and glibc (tests/test_gpu_ops.py, pairwise IoU against the golden values)
CPU_TABLE_BOUND = 5e-5      # oracle against the closed forms of the degenerate table, tests/test_bev_iou_refs_cpu.py


def dev():
    assert torch.cuda.is_available(), 'gpu-marked tests need the MI355X'
    return torch.device('cuda:0')


def _ops():
    from pcp_amd import ops
    return ops


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())


def _nms(fn):
    return _ops().nms_normal if fn == 'normal' else _ops().nms_rotated


def _iou_fn(fn):
    return onms.iou_normal_matrix if fn == 'normal' else onms.iou_matrix


def _kept(keep, cnt, b=None):
    """(keep list as int64 numpy, the zero tail is checked)"""
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    row, n = (keep, int(cnt[0])) if b is None else (keep[b], int(cnt[b]))
    assert 0 <= n <= row.shape[0]
    assert (row[n:] == 0).all(), 'keep beyond count must stay zero'
    return row[:n].astype(np.int64)


# ---- a. pairwise against float64 -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pairwise_case(na, nb):
    boxes = R.clustered(11, na + nb)
    a, b = boxes[:na], boxes[na:]
    big = np.maximum((a[:, 3] * a[:, 4])[:, None], (b[:, 3] * b[:, 4])[None, :]).astype(np.float64)
    return dict(a=a, b=b, big=big, clear=R.clearance64(a, b), iou64=R.iou64(a, b), ov64=R.overlap64(a, b),
                iou_o=onms.iou_matrix(a, b).astype(np.float64), ov_o=onms.overlap_matrix(a, b).astype(np.float64))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('na,nb', [(37, 130), (1, 64), (64, 1), (65, 65)])
def test_pairwise_against_float64_and_oracle(na, nb, mode):
    c = _pairwise_case(na, nb)
    got = _ops().boxes_bev_pairwise(_t(c['a']), _t(c['b']), mode).cpu().numpy().astype(np.float64)
    assert got.shape == (na, nb) and np.isfinite(got).all()
    ref64, ref_o = (c['iou64'], c['iou_o']) if mode == 1 else (c['ov64'], c['ov_o'])
    scale = np.ones_like(c['big']) if mode == 1 else c['big']              # mode 0: relative to the larger box area
    generic = c['clear'] >= R.GENERIC_CLEARANCE
    oracle_dev = float((np.abs(ref_o - ref64) / scale)[generic].max()) if generic.any() else 0.0      # from the oracle, not from the kernel
    err64 = np.abs(got - ref64) / scale
    err_o = np.abs(got - ref_o) / scale
    # against the oracle on every pair; a pair may only leave the allowance when a corner sits on the margin itself (a corner_in verdict
    # flipped by an ulp of sinf / cosf)
    over = err_o > GPU_VS_ORACLE
    on_margin = np.abs(c['clear'] - R.NMS_MARGIN) <= 1e-5
    left_out = np.argwhere(over & on_margin)
    print('pairwise (%d, %d) mode %d: GPU vs float64 on %d generic pairs %.3g (oracle vs float64 %.3g), GPU vs oracle on all pairs %.3g, '
          '%d margin pairs left out' % (na, nb, mode, generic.sum(), err64[generic].max() if generic.any() else 0.0, oracle_dev,
                                        err_o[~(over & on_margin)].max(), left_out.shape[0]))
    assert (err64[generic] <= oracle_dev + GPU_VS_ORACLE).all(), np.argwhere(generic & (err64 > oracle_dev + GPU_VS_ORACLE))[:10]
    bad = np.argwhere(over & ~on_margin)
    assert bad.shape[0] == 0, [(i, j, got[i, j], ref_o[i, j], c['clear'][i, j]) for i, j in bad[:10]]
    assert left_out.shape[0] <= 0.005 * na * nb, [(i, j, got[i, j], ref_o[i, j], c['clear'][i, j]) for i, j in left_out]


# ---- b. the degenerate table -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _table():
    a, b, exact_iou, exact_ov, kind = R.degenerate_table()
    k = np.arange(a.shape[0])
    return a, b, exact_iou, exact_ov, kind, onms.iou_matrix(a, b)[k, k].astype(np.float64), onms.overlap_matrix(a, b)[k, k].astype(np.float64)


@pytest.mark.parametrize('mode', [0, 1])
def test_degenerate_table_against_closed_forms_and_oracle(mode):
    a, b, exact_iou, exact_ov, kind, iou_o, ov_o = _table()
    k = np.arange(a.shape[0])
    got = _ops().boxes_bev_pairwise(_t(a), _t(b), mode).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                          # the cross pairs of the table too
    got = got[k, k]
    exact, ref_o = (exact_iou, iou_o) if mode == 1 else (exact_ov, ov_o)
    scale = 1.0 if mode == 1 else np.maximum(np.maximum(a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]).astype(np.float64), 1.0)
    e_exact, e_o = np.abs(got - exact) / scale, np.abs(got - ref_o) / scale
    print('degenerate table mode %d: GPU vs closed form %.3g (%s), GPU vs oracle %.3g (%s)'
          % (mode, e_exact.max(), kind[int(e_exact.argmax())], e_o.max(), kind[int(e_o.argmax())]))
    assert (e_exact <= CPU_TABLE_BOUND + GPU_VS_ORACLE).all(), [(kind[i], got[i], exact[i]) for i in np.argwhere(e_exact > CPU_TABLE_BOUND + GPU_VS_ORACLE)[:, 0]]
    assert (e_o <= GPU_VS_ORACLE).all(), [(kind[i], got[i], ref_o[i]) for i in np.argwhere(e_o > GPU_VS_ORACLE)[:, 0]]


def test_tiny_boxes_follow_the_oracle_above_one():
    """boxes of the size of NMS_MARGIN: the reference arithmetic returns IoU > 1 and the kernel follows it (not float64)"""
    a, b = R.tiny_pairs()
    k = np.arange(a.shape[0])
    for mode, ref in ((1, onms.iou_matrix(a, b)[k, k]), (0, onms.overlap_matrix(a, b)[k, k])):
        got = _ops().boxes_bev_pairwise(_t(a), _t(b), mode).cpu().numpy()[k, k]
        assert np.isfinite(got).all()
        assert np.abs(got.astype(np.float64) - ref).max() <= GPU_VS_ORACLE
        if mode == 1:
            assert (got > 1.15).all()


# ---- c. batched, ragged, pre-sorted: the production call shape -------------------------------------------------------------------------

N_MAX = 200
N_DEV = [200, 0, 1, 65, 130, 64]


@functools.lru_cache(maxsize=None)
def _frames(fn):
    """(6, 200, 7) boxes, every frame threshold-safe under the IoU of fn; row order is score order"""
    out = []
    for b in range(len(N_DEV)):
        safe = R.threshold_safe(R.clustered(20 + b, 240), THR, 1e-4, _iou_fn(fn))
        assert safe.shape[0] >= N_MAX
        out.append(safe[:N_MAX])
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _frame_hits(fn):
    return [_iou_fn(fn)(f, f) > THR for f in _frames(fn)]


@pytest.mark.parametrize('variant', ['base', 'clamped_counts', 'pre_max_50', 'post_max_30'])
@pytest.mark.parametrize('fn', ['rotated', 'normal'])
def test_batched_ragged_presorted_frames(fn, variant):
    n_dev = [250, -3] + N_DEV[2:] if variant == 'clamped_counts' else list(N_DEV)
    pre_max = 50 if variant == 'pre_max_50' else 1000
    post_max = 30 if variant == 'post_max_30' else N_MAX
    n_true = [min(max(n, 0), N_MAX) for n in n_dev]
    B = len(n_dev)
    boxes = _frames(fn).copy()
    scores = np.tile(np.linspace(0.9, 0.1, N_MAX, dtype=np.float32), (B, 1))               # strictly descending
    for b in range(B):
        boxes[b, n_true[b]:] = np.nan                                      # rows beyond the count are never read
        scores[b, n_true[b]:] = np.nan
    want = [R.greedy_nms(_frame_hits(fn)[b][:min(n_true[b], pre_max), :min(n_true[b], pre_max)], post_max) for b in range(B)]
    assert [w.shape[0] for w in want][1:3] == [0, 1] and 10 < want[4].shape[0] < n_true[4]                 # the threshold bites
    nms = _nms(fn)
    nd = _t(np.asarray(n_dev, np.int32))
    keep, cnt = nms(_t(boxes), None, THR, pre_max, post_max, n_dev=nd)
    keep_s, cnt_s = nms(_t(boxes), _t(scores), THR, pre_max, post_max, n_dev=nd)
    torch.cuda.synchronize()
    assert keep.shape == (B, post_max) and cnt.shape == (B,)
    for b in range(B):
        got = _kept(keep, cnt, b)
        assert np.array_equal(got, want[b]), 'frame %d' % b
        assert np.array_equal(_kept(keep_s, cnt_s, b), got), 'frame %d: the sort path on strictly descending scores is the identity path' % b
        one, one_cnt = nms(_t(boxes[b, :n_true[b]]).reshape(n_true[b], 7), None, THR, pre_max, post_max)
        assert np.array_equal(_kept(one, one_cnt), got), 'frame %d: the single-frame call' % b


# ---- d. structural sweep cases ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _chain(n):
    return R.chain_line(n)


@pytest.mark.parametrize('fn', ['rotated', 'normal'])
@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('n', [64, 65, 128, 129, 4096])
def test_chain_line_keeps_every_other_box(n, permuted, fn):
    boxes, hit = _chain(n)
    nms = _nms(fn)
    if not permuted:
        want = np.arange(0, n, 2)
        keep, cnt = nms(_t(boxes), None, THR, n, n)
        assert np.array_equal(_kept(keep, cnt), want)
        keep, cnt = nms(_t(boxes), _t(np.linspace(1.0, 0.0, n, dtype=np.float32)), THR, n, n)
        assert np.array_equal(_kept(keep, cnt), want)
        return
    scores = np.random.RandomState(n).permutation(n).astype(np.float32)
    order = R.stable_desc_order(scores)
    want_sorted = R.greedy_nms(hit[order][:, order])
    assert not np.array_equal(order[want_sorted], np.arange(0, n, 2))
    keep, cnt = nms(_t(boxes), _t(scores), THR, n, n)
    assert np.array_equal(_kept(keep, cnt), order[want_sorted])
    keep, cnt = nms(_t(boxes[order]), None, THR, n, n)                     # the same order handed in pre-sorted
    assert np.array_equal(_kept(keep, cnt), want_sorted)


@pytest.mark.parametrize('fn', ['rotated', 'normal'])
@pytest.mark.parametrize('case', ['duplicates_across_blocks', 'three_block_chain'])
def test_cross_block_suppression(case, fn):
    boxes, want = getattr(R, case)()
    n = boxes.shape[0]
    nms = _nms(fn)
    keep, cnt = nms(_t(boxes), None, THR, n, n)
    assert np.array_equal(_kept(keep, cnt), want)
    keep, cnt = nms(_t(boxes), _t(np.linspace(1.0, -1.0, n, dtype=np.float32)), THR, n, n)
    assert np.array_equal(_kept(keep, cnt), want)


@pytest.mark.parametrize('post_max', [1, 64, 65, 128, 200, 500])
def test_post_max_on_a_set_without_overlap(post_max):
    n = 200
    boxes = R.far_apart_grid(n, seed=3)
    scores = np.random.RandomState(5).permutation(n).astype(np.float32)
    order = R.stable_desc_order(scores)
    m = min(n, post_max)
    keep, cnt = _ops().nms_rotated(_t(boxes), _t(scores), THR, 1000, post_max)
    assert keep.shape == (post_max,) and int(cnt[0]) == m
    assert np.array_equal(_kept(keep, cnt), order[:m])
    keep, cnt = _ops().nms_rotated(_t(boxes), None, THR, 1000, post_max)
    assert np.array_equal(_kept(keep, cnt), np.arange(m))


@pytest.mark.parametrize('post_max', [32, 33, 34, 65])
def test_post_max_cut_on_a_block_edge(post_max):
    """one isolated box, then chain_line(255): rows 0, 1, 3, 5, ... are kept, so block 0 ends on a kept row (63) holding the 33rd kept box and
    block 1 on row 127 holding the 65th"""
    chain, _hit = R.chain_line(255)
    first = chain[:1].copy()
    first[0, 1] = 50.0
    boxes = np.concatenate([first, chain])
    full = np.concatenate([[0], np.arange(1, 256, 2)])
    assert full[32] == 63 and full[64] == 127
    for fn in ('rotated', 'normal'):
        keep, cnt = _nms(fn)(_t(boxes), None, THR, 256, post_max)
        assert np.array_equal(_kept(keep, cnt), full[:post_max])


@pytest.mark.parametrize('fill', [0xFF, 0x00])
def test_result_does_not_depend_on_workspace_contents(fill):
    ops = _ops()
    from pcp_amd import lib
    d = dev()
    # single frame, through the sort
    boxes = _frames('rotated')[0]
    scores = np.random.RandomState(9).permutation(N_MAX).astype(np.float32)
    order = R.stable_desc_order(scores)
    want = order[R.greedy_nms(_frame_hits('rotated')[0][order][:, order])]
    need = int(lib.load().pcp_nms_workspace_bytes(N_MAX, 1))
    ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device=d)
    keep, cnt = ops.nms_rotated(_t(boxes), _t(scores), THR, 1000, N_MAX, workspace=ws)
    fresh, fresh_cnt = ops.nms_rotated(_t(boxes), _t(scores), THR, 1000, N_MAX)
    assert np.array_equal(_kept(keep, cnt), want) and torch.equal(keep, fresh) and torch.equal(cnt, fresh_cnt)
    # batched and ragged, pre-sorted
    B = len(N_DEV)
    nd = _t(np.asarray(N_DEV, np.int32))
    need = int(lib.load().pcp_nms_workspace_bytes(N_MAX, B))
    ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device=d)
    keep, cnt = ops.nms_rotated(_t(_frames('rotated')), None, THR, 1000, N_MAX, n_dev=nd, workspace=ws)
    fresh, fresh_cnt = ops.nms_rotated(_t(_frames('rotated')), None, THR, 1000, N_MAX, n_dev=nd)
    assert torch.equal(keep, fresh) and torch.equal(cnt, fresh_cnt)
    for b in range(B):
        assert np.array_equal(_kept(keep, cnt, b), R.greedy_nms(_frame_hits('rotated')[b][:N_DEV[b], :N_DEV[b]]))


# ---- e. the sort -----------------------------------------------------------------------------------------------------------------------

def _sorted_order_through_nms(scores):
    """NMS on boxes that never overlap keeps everything, in sort order"""
    n = scores.shape[0]
    keep, cnt = _ops().nms_rotated(_t(R.far_apart_grid(n, seed=n)), _t(scores), THR, n, n)
    assert int(cnt[0]) == n
    return _kept(keep, cnt)


@pytest.mark.parametrize('n', [2, 64, 65, 1000, 4096])
def test_sort_is_the_stable_descending_order_with_ties_negatives_and_infinities(n):
    values = np.array([-np.inf, -2.5, -1.0, -1e-30, -1e-40, 1e-40, 1e-30, 0.5, 0.75, 3.0, np.inf], np.float32)
    scores = values[np.random.RandomState(n).randint(0, values.shape[0], n)]
    if n == 2:
        scores = np.array([-1.0, -1.0], np.float32)
    assert np.unique(scores).shape[0] < max(n, 2)                          # ties
    assert np.array_equal(_sorted_order_through_nms(scores), R.stable_desc_order(scores))


@pytest.mark.parametrize('n', [2, 64, 65, 1000, 4096])
def test_sort_takes_both_zeros_as_equal(n):
    """the reference sorts with a float comparison, under which -0.0 == +0.0: they stay in index order"""
    values = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32)
    scores = values[np.random.RandomState(100 + n).randint(0, values.shape[0], n)]
    if n == 2:
        scores = np.array([-0.0, 0.0], np.float32)
    assert np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    assert np.array_equal(_sorted_order_through_nms(scores), R.stable_desc_order(scores))


# ---- f. limits -------------------------------------------------------------------------------------------------------------------------

def test_two_frames_of_4096():
    n = 4096
    chain, _hit = _chain(n)
    boxes = np.stack([chain, R.far_apart_grid(n, seed=1)])
    n_dev = [n, 4000]
    boxes[1, 4000:] = np.nan
    want = [np.arange(0, n, 2), np.arange(4000)]
    scores = np.tile(np.linspace(1.0, 0.0, n, dtype=np.float32), (2, 1))
    nd = _t(np.asarray(n_dev, np.int32))
    for sc in (None, _t(scores)):
        keep, cnt = _ops().nms_rotated(_t(boxes), sc, THR, n, n, n_dev=nd)
        for b in range(2):
            assert np.array_equal(_kept(keep, cnt, b), want[b])


def test_limits_raise_or_return_empty():
    from pcp_amd import lib
    ops = _ops()

    def status(code):
        return lib.load().pcp_status_string(code).decode()

    unsupported, bad_arg = status(4), status(1)                            # PCP_ERR_UNSUPPORTED, PCP_ERR_ARG of include/pcp_hip.h
    assert unsupported != bad_arg
    big = _t(R.far_apart_grid(4097))
    with pytest.raises(lib.PcpError) as e:
        ops.nms_rotated(big, None, THR, 4097, 100)
    assert unsupported in str(e.value)
    with pytest.raises(lib.PcpError) as e:
        ops.nms_normal(big.reshape(1, 4097, 7), _t(np.zeros((1, 4097), np.float32)), THR, 4097, 100)
    assert unsupported in str(e.value)
    small = _t(R.far_apart_grid(10))
    for pre_max, post_max in ((0, 10), (10, 0)):
        with pytest.raises(lib.PcpError) as e:
            ops.nms_rotated(small, None, THR, pre_max, post_max)
        assert bad_arg in str(e.value)
    keep, cnt = ops.nms_rotated(torch.zeros((3, 0, 7), dtype=torch.float32, device=dev()), None, THR, 100, 10,
                                n_dev=_t(np.asarray([0, 5, -1], np.int32)))
    assert cnt.cpu().tolist() == [0, 0, 0] and int(keep.abs().sum()) == 0
