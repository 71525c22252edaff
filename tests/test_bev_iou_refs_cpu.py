"""tests/bev_iou_refs.py checked on the CPU: the float64 clipper against closed forms, the project's float32 oracle (oracle/nms_oracle.c, the
restatement of the reference arithmetic that csrc/bev_geom.h follows) against the clipper on generic pairs and on the degenerate table, the
numpy greedy sweep against the oracle's, and the structural NMS builders against the keep lists their docstrings claim.  No GPU."""
import numpy as np
import pytest

import bev_iou_refs as R
from oracle import nms as onms


def _oracle_rows(a, b):
    iou = np.array([onms.iou_matrix(a[k:k + 1], b[k:k + 1])[0, 0] for k in range(a.shape[0])], np.float64)
    ov = np.array([onms.overlap_matrix(a[k:k + 1], b[k:k + 1])[0, 0] for k in range(a.shape[0])], np.float64)
    return iou, ov


# ---- the clipper itself ----------------------------------------------------------------------------------------------------------------

def test_float64_clipper_gives_the_closed_forms_of_the_degenerate_table():
    a, b, exact_iou, exact_ov, kind = R.degenerate_table()
    assert len(kind) == 3 * 8 * 10
    iou, ov = R.iou64(a, b, rows=True), R.overlap64(a, b, rows=True)
    assert np.isfinite(iou).all() and np.isfinite(ov).all()
    # the only error is the float32 rounding of the inputs (centre + shift at 100 m: 8e-6 m on a 2 m edge; ang + pi: 2e-7 rad on a 4 m box)
    print('clipper vs closed form: IoU %.3g, overlap %.3g m^2' % (np.abs(iou - exact_iou).max(), np.abs(ov - exact_ov).max()))
    assert np.abs(iou - exact_iou).max() <= 2e-6            # measured 6.2e-7
    assert np.abs(ov - exact_ov).max() <= 2e-5              # measured 5.6e-6
    exact_rows = np.array([k in ('identical', 'concentric', 'turned_inside', 'crossed', 'far', 'zero_zero', 'zero_in_2x2') for k in kind])
    assert np.abs(iou - exact_iou)[exact_rows].max() <= 1e-12          # no rounded shift or heading in these rows


def test_float64_clipper_is_symmetric_bounded_and_invariant_under_a_rigid_move():
    b = R.clustered(5, 90)
    ov = R.overlap64(b, b)
    area = b[:, 3].astype(np.float64) * b[:, 4]
    assert np.abs(ov - ov.T).max() <= 1e-12
    assert (ov <= np.minimum(area[:, None], area[None, :]) + 1e-12).all() and (ov >= 0).all()
    assert np.abs(np.diag(ov) - area).max() <= 1e-12
    th, sx, sy = 0.7, 3.0, -11.0                                           # the same scene turned and shifted, in float64
    b = b.astype(np.float64)
    m = b.copy()
    m[:, 0] = np.cos(th) * b[:, 0] - np.sin(th) * b[:, 1] + sx
    m[:, 1] = np.sin(th) * b[:, 0] + np.cos(th) * b[:, 1] + sy
    m[:, 6] = b[:, 6] + th
    assert np.abs(R.overlap64(m, m) - ov).max() <= 1e-11
    assert np.abs(R.clearance64(m, m) - R.clearance64(b, b)).max() <= 1e-11


def test_corners_and_clearance_on_hand_cases():
    c = R.corners64(np.array([[1.0, 2.0, 0, 4.0, 2.0, 1, np.pi / 2]]))[0]
    assert np.abs(c - np.array([[2.0, 0.0], [2.0, 4.0], [0.0, 4.0], [0.0, 0.0]])).max() <= 1e-15
    a = np.array([[0.0, 0.0, 0, 4.0, 2.0, 1, 0.0]])
    for bx, want in (([5.0, 0.0, 0, 4.0, 2.0, 1, 0.0], 1.0),               # 1 m gap along x
                     ([1.0, 0.0, 0, 4.0, 2.0, 1, 0.0], 0.0),               # corners on the other box's (extended) edges
                     ([0.0, 0.0, 0, 1.0, 1.0, 1, 0.0], 0.5),               # inside: nearest edge 0.5 m away
                     ([5.0, 4.0, 0, 2.0, 2.0, 1, 0.0], np.hypot(2.0, 2.0))):     # corner to corner
        assert abs(R.clearance64(a, np.array([bx]))[0, 0] - want) <= 1e-15


# ---- the oracle against float64 --------------------------------------------------------------------------------------------------------

def test_oracle_matches_float64_on_generic_clustered_pairs():
    boxes = R.clustered(1, 200)
    near = R.near_pairs(boxes, boxes) & ~np.eye(200, dtype=bool)
    generic = R.clearance64(boxes, boxes) >= R.GENERIC_CLEARANCE
    share = (near & ~generic).sum() / near.sum()
    d_iou = np.abs(onms.iou_matrix(boxes, boxes) - R.iou64(boxes, boxes))[generic].max()
    d_ov = np.abs(onms.overlap_matrix(boxes, boxes) - R.overlap64(boxes, boxes))[generic].max()
    print('clustered(1, 200): %d near pairs, %.1f %% of them non-generic and left out; oracle vs float64 on the rest: IoU %.3g, overlap %.3g m^2'
          % (near.sum(), 100 * share, d_iou, d_ov))
    assert near.sum() >= 2000
    assert share <= 0.10                      # measured 8.2 %
    assert d_iou <= 1.2e-5                    # measured 2.8e-6, x4 for seed changes
    assert d_ov <= 1.0e-4                     # measured 2.35e-5 m^2, x4


def test_oracle_matches_the_closed_forms_of_the_degenerate_table():
    a, b, exact_iou, exact_ov, kind = R.degenerate_table()
    iou, ov = _oracle_rows(a, b)
    assert np.isfinite(iou).all() and np.isfinite(ov).all()
    worst = int(np.abs(iou - exact_iou).argmax())
    print('oracle vs closed form: IoU %.3g (%s), overlap %.3g m^2' % (np.abs(iou - exact_iou).max(), kind[worst], np.abs(ov - exact_ov).max()))
    assert np.abs(iou - exact_iou).max() <= 5e-5                                     # measured 1.7e-5 (identical boxes at (-100.4, 99.9))
    big = np.maximum(a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]).astype(np.float64)
    assert (np.abs(ov - exact_ov) <= 5e-5 * np.maximum(big, 1.0)).all()            # measured 6.7e-5 m^2 on 7.98 m^2


def test_margin_quirk_boxes_of_centimetre_size_have_oracle_iou_above_one():
    """why centimetre boxes are compared with the oracle and not with float64: every corner is within NMS_MARGIN of the other square"""
    a, b = R.tiny_pairs()
    iou, _ov = _oracle_rows(a, b)
    true = R.iou64(a, b, rows=True)
    print('tiny pairs: oracle IoU %s, float64 IoU %s' % (np.round(iou, 4), np.round(true, 4)))
    assert (iou > 1.15).all() and (iou < 1.25).all()
    assert np.abs(true[0::2] - 9 / 11).max() <= 2e-4 and np.abs(true[1::2] - 81 / 119).max() <= 3e-4      # float32 shift of 0.005 at 100 m
    assert (R.clearance64(a, b, rows=True) < R.GENERIC_CLEARANCE).all()


# ---- the sweep, the sort, the builders ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_greedy_nms_equals_the_oracle_sweep(n):
    rng = np.random.RandomState(n)
    for density in (0.0, 0.02, 0.3, 1.0):
        hit = rng.uniform(size=(n, n)) < density
        want = onms.nms_from_iou(hit.astype(np.float32), 0.5)
        assert np.array_equal(R.greedy_nms(hit), want)
        for post_max in (1, 7, n, n + 3):
            assert np.array_equal(R.greedy_nms(hit, post_max), want[:post_max])


def test_stable_desc_order_holds_ties_in_index_order_and_both_zeros_equal():
    s = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 1.0, np.inf, -np.inf], np.float32)
    assert R.stable_desc_order(s).tolist() == [7, 2, 6, 0, 1, 3, 4, 5, 8]


@pytest.mark.parametrize('fn', ['rotated', 'normal'])
def test_threshold_safe_leaves_the_stated_gap(fn):
    iou_fn = onms.iou_matrix if fn == 'rotated' else onms.iou_normal_matrix
    boxes = R.clustered(3, 400)
    for thr, gap in ((0.2, 1e-4), (0.2, 2e-3)):
        safe = R.threshold_safe(boxes, thr, gap, iou_fn)
        iou = iou_fn(safe, safe).astype(np.float64)
        off = ~np.eye(safe.shape[0], dtype=bool)
        assert (np.abs(iou - thr)[off] >= gap).all()
        assert 300 <= safe.shape[0] <= 400
        assert np.array_equal(R.threshold_safe(boxes, thr, gap, iou_fn), safe)                 # deterministic
    assert R.threshold_safe(boxes, 0.2, 2e-3, iou_fn).shape[0] < 400                           # the wide gap does drop some


def _keep_by_float64_and_oracle(boxes, thr):
    i64 = R.iou64(boxes, boxes)
    io = onms.iou_matrix(boxes, boxes)
    assert np.abs(i64 - thr).min() > 0.05 and np.abs(io - thr).min() > 0.05, 'every verdict is far from the threshold'
    k64, ko = R.greedy_nms(i64 > thr), R.greedy_nms(io > thr)
    assert np.array_equal(k64, ko)
    return k64


@pytest.mark.parametrize('n', [64, 65, 129])
def test_chain_line_keeps_every_other_box(n):
    boxes, hit = R.chain_line(n)
    i64 = R.iou64(boxes, boxes)
    assert np.array_equal(i64 > 0.2, hit | np.eye(n, dtype=bool))
    assert np.abs(i64[hit] - 0.28).max() <= 1e-12 and (i64[~hit & ~np.eye(n, dtype=bool)] == 0).all()
    assert np.array_equal(onms.iou_normal_matrix(boxes, boxes) > 0.2, hit | np.eye(n, dtype=bool))
    assert np.array_equal(_keep_by_float64_and_oracle(boxes, 0.2), np.arange(0, n, 2))
    assert np.array_equal(R.greedy_nms(hit), np.arange(0, n, 2))


def test_chain_line_is_exact_in_float32_at_its_far_end():
    boxes, hit = R.chain_line(4096)
    assert np.array_equal(boxes[:, 0].astype(np.float64), 2.25 * np.arange(4096))
    tail = boxes[-130:]
    assert np.array_equal(onms.iou_matrix(tail, tail) > 0.2, hit[-130:, -130:] | np.eye(130, dtype=bool))


def test_duplicates_across_blocks_and_three_block_chain_have_their_keep_lists():
    boxes, keep = R.duplicates_across_blocks()
    assert boxes.shape == (266, 7) and keep.shape[0] == 260
    gone = np.setdiff1d(np.arange(266), keep)
    assert (gone // 64).tolist() == [0, 1, 1, 2, 3, 4] and (boxes[gone] == boxes[5]).all()
    assert np.array_equal(_keep_by_float64_and_oracle(boxes, 0.2), keep)
    boxes, keep = R.three_block_chain()
    assert np.array_equal(_keep_by_float64_and_oracle(boxes, 0.2), keep)
    assert np.setdiff1d(np.arange(192), keep).tolist() == [84]
    i64 = R.iou64(boxes[[10, 84, 158]], boxes[[10, 84, 158]])
    assert i64[0, 1] > 0.25 and i64[1, 2] > 0.25 and i64[0, 2] == 0


def test_far_apart_grid_has_no_overlap():
    for n in (2, 200, 4096):
        b = R.far_apart_grid(n, seed=n)
        assert R.near_pairs(b, b).sum() == n                               # only each box with itself
