"""The float64 reference, the restated split plans and the case tables of tests/wgrad3x3_refs.py, checked on the CPU: the reference against
torch's float64 autograd, the integer variants against the condition that makes bit-equality owed, and every case's `why` against the plan
(computed from the kernels' documented constants, not from the kernels).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad3x3_refs as wr

CASES = [(k, i) for k in ('fp32', 'bf16') for i in range(len(wr.TABLES[k]))]


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _autograd_dw(x, dy, stride):
    cin, cout = x.shape[3], dy.shape[3]
    w = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(_t(x).permute(0, 3, 1, 2), w, None, stride=stride, padding=1).backward(_t(dy).permute(0, 3, 1, 2))
    return w.grad.numpy()


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,i', CASES)
def test_reference_equals_float64_autograd_and_S_dominates(kind, i):
    c, d = wr.TABLES[kind][i], wr.case_data(kind, i, False)
    want = _autograd_dw(d['x'], d['dy'], c.stride)
    assert d['dw'].shape == want.shape == (c.cout, c.cin, 3, 3)
    assert np.allclose(d['dw'], want, rtol=1e-12, atol=1e-12 * float(d['S'].max()))
    assert (d['S'] >= np.abs(d['dw'])).all()
    Ho, Wo = wr.out_hw(c.H, c.W, c.stride)
    assert d['K'] == c.B * Ho * Wo and d['dy'].shape == (c.B, Ho, Wo, c.cout)
    # S is the same operation on the absolute values
    S = _autograd_dw(np.abs(d['x']), np.abs(d['dy']), c.stride)
    assert np.allclose(d['S'], S, rtol=1e-12, atol=0)


def test_reference_from_the_definition_on_a_small_map():
    """the formula of the header, one term at a time, at both strides (an odd-sized map at stride 1)"""
    for stride, (B, H, W) in ((1, (2, 3, 5)), (2, (2, 4, 6))):
        Ho, Wo = wr.out_hw(H, W, stride)
        x, dy = wr.uniform(801, 1, (B, H, W, 3)), wr.uniform(801, 2, (B, Ho, Wo, 2))
        dw = np.zeros((2, 3, 3, 3))
        for b in range(B):
            for oy in range(Ho):
                for ox in range(Wo):
                    for ky in range(3):
                        for kx in range(3):
                            iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
                            if 0 <= iy < H and 0 <= ix < W:
                                dw[:, :, ky, kx] += np.outer(wr.f64(dy[b, oy, ox]), wr.f64(x[b, iy, ix]))
        assert float(np.abs(wr.wgrad3x3(x, dy, stride)[0] - dw).max()) <= 1e-13


@pytest.mark.parametrize('kind,i', CASES)
def test_integer_variants_make_every_partial_sum_exact(kind, i):
    """non-zero integers of magnitude <= 8, and sum |dy| |x| < 2^22: every partial sum of every order is an integer below 2^24"""
    c, d = wr.TABLES[kind][i], wr.case_data(kind, i, True)
    for a in (d['x'], d['dy']):
        assert a.dtype == np.float32 and (a != 0).all() and np.abs(a).max() <= wr.INT_MAX and np.array_equal(a, np.round(a))
        assert np.array_equal(wr.bf16_round(a), a)
    if d['x'].size >= 4096:
        assert len(np.unique(d['x'])) == 2 * wr.INT_MAX and len(np.unique(d['dy'])) == 2 * wr.INT_MAX
    assert float(d['S'].max()) < 2.0 ** 22
    assert np.array_equal(d['dw'], np.round(d['dw'])) and np.array_equal(d['dw'].astype(np.float32).astype(np.float64), d['dw'])
    assert c.B * c.H * c.W * c.cin + d['dy'].size <= 3.1e6                     # a few seconds per case


def test_float_variants_of_the_bf16_table_are_exact_in_bf16():
    d = wr.case_data('bf16', 3, False)
    for a in (d['x'], d['dy']):
        assert torch.equal(torch.from_numpy(np.array(a)).bfloat16().float(), torch.from_numpy(np.array(a)))
    a = wr.uniform(802, 1, (4096,), -3.0, 3.0)
    assert torch.equal(torch.from_numpy(wr.bf16_round(a)), torch.from_numpy(a).bfloat16().float())          # ties to even, as torch rounds
    ties = np.array([1.00390625, 1.01171875, -1.00390625], np.float32)                                        # 1 + 2^-8, 1 + 3 * 2^-8
    assert wr.bf16_round(ties).tolist() == [1.0, 1.015625, -1.0]


def test_case_data_is_cached_and_read_only():
    d = wr.case_data('fp32', 0, True)
    assert wr.case_data('fp32', 0, True) is d
    with pytest.raises(ValueError):
        d['x'][0, 0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        wr.place_x('bf16', 2)[0, 0, 0, 0] = 1.0


# ---- the one-hot expectation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,stride', sorted(wr.PLACE))
def test_one_hot_expectation_equals_the_reference(kind, stride):
    c, x = wr.PLACE[(kind, stride)], wr.place_x(kind, stride)
    Ho, Wo = wr.out_hw(c.H, c.W, stride)
    assert (x != 0).all()
    pixels = wr.place_pixels(kind, stride)
    assert {b for _w, b, _y, _x in pixels} == set(range(c.B))
    for n, (what, b, oy, ox) in enumerate(pixels):
        co = n % c.cout
        dy = np.zeros((c.B, Ho, Wo, c.cout), np.float32)
        dy[b, oy, ox, co] = 1.0
        dw, _S = wr.wgrad3x3(x, dy, stride)
        want = wr.one_hot_expect(x, b, oy, ox, stride)
        assert np.array_equal(dw[co], want), what
        assert not dw[np.arange(c.cout) != co].any()
        outside = [(ky, kx) for ky in range(3) for kx in range(3)
                   if not (0 <= oy * stride + ky - 1 < c.H and 0 <= ox * stride + kx - 1 < c.W)]
        assert all(not want[:, ky, kx].any() for ky, kx in outside) and (want != 0).sum() == c.cin * (9 - len(outside))
        if what == 'corner' and (oy, ox) == (0, 0):
            assert len(outside) == 5
        if what == 'interior':
            assert not outside


def test_placement_pixels_straddle_the_boundaries_of_the_plans():
    for (kind, stride), c in wr.PLACE.items():
        Ho, Wo = wr.out_hw(c.H, c.W, stride)
        px = {(oy, ox) for _w, _b, oy, ox in wr.place_pixels(kind, stride)}
        assert {(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)} <= px
        if kind == 'fp32':
            by, bx = wr.tile_fp32(stride)
            ty, tx, _n, _ns = wr.plan_fp32(*c[:6])
            assert ty >= 2 and tx >= 2
        else:
            n_strips, n_rsplit, by, _n = wr.plan_bf16(*c[:6])
            bx = wr.WG_DW
            assert n_strips >= 2 and n_rsplit >= 2
        assert {oy // by for oy, _ in px} >= {0, 1} and {ox // bx for _, ox in px} >= {0, 1}
        assert any(oy == by - 1 for oy, _ in px) and any(oy == by for oy, _ in px)
        assert any(ox == bx - 1 for _, ox in px) and any(ox == bx for _, ox in px)


# ---- the plans, restated a second time from the rule, and what every case claims ----------------------------------------------------------

@pytest.mark.parametrize('i', range(len(wr.FP32_CASES)))
def test_plan_fp32_is_the_rule(i):
    c = wr.FP32_CASES[i]
    Ho, Wo = c.H // c.stride, c.W // c.stride
    th, tw = (8, 16) if c.stride == 1 else (4, 8)
    ty, tx = (Ho + th - 1) // th, (Wo + tw - 1) // tw
    pairs = ((c.cout + 63) // 64) * ((c.cin + 63) // 64)
    assert wr.plan_fp32(*c[:6]) == (ty, tx, c.B * ty * tx, max(1, min(256 // pairs, c.B * ty * tx)))
    assert c.cin % 4 == 0 and c.cout % 4 == 0 and (c.stride == 1 or (c.H % 2 == 0 and c.W % 2 == 0))
    assert sum(wr.trips_fp32(*c[:6])) == c.B * ty * tx


@pytest.mark.parametrize('i', range(len(wr.BF16_CASES)))
def test_plan_bf16_is_the_rule(i):
    c = wr.BF16_CASES[i]
    Ho, Wo = c.H // c.stride, c.W // c.stride
    tr = 4 if c.stride == 1 else 2
    n_strips = (Wo + 31) // 32
    base = c.B * n_strips * ((c.cout + 63) // 64) * ((c.cin + 63) // 64)
    rsplit = min((256 + base // 2) // base, (Ho + 2 * tr - 1) // (2 * tr))
    rsplit = max(rsplit, 1)
    per = (Ho + rsplit - 1) // rsplit
    rows_per = (per + tr - 1) // tr * tr
    n_rsplit = (Ho + rows_per - 1) // rows_per
    assert wr.plan_bf16(*c[:6]) == (n_strips, n_rsplit, rows_per, c.B * n_strips * n_rsplit)
    assert c.cin % 8 == 0 and c.cout % 8 == 0 and (c.stride == 1 or (c.H % 2 == 0 and c.W % 2 == 0))
    st = wr.stages_bf16(*c[:6])
    assert len(st) == n_rsplit and all(s >= 1 for s in st) and rows_per % tr == 0
    assert sum(min(rows_per, Ho - r * rows_per) for r in range(n_rsplit)) == Ho


def _fp32(*shape):
    i = wr.index_of('fp32', *shape)
    return wr.FP32_CASES[i], wr.plan_fp32(*shape), wr.trips_fp32(*shape)


def test_fp32_cases_reach_the_paths_they_name():
    assert len({tuple(c[:6]) for c in wr.FP32_CASES}) == len(wr.FP32_CASES) and all(c.why for c in wr.FP32_CASES)
    c, plan, trips = _fp32(1, 1, 1, 8, 8, 1)
    assert plan == (1, 1, 1, 1)
    c, plan, trips = _fp32(1, 8, 16, 64, 64, 1)
    assert plan == (1, 1, 1, 1) and (c.H, c.W) == wr.tile_fp32(1)                           # exactly one full tile
    c, plan, trips = _fp32(1, 9, 17, 4, 4, 1)
    assert plan == (2, 2, 4, 4) and c.H % 8 == 1 and c.W % 16 == 1                         # three tiles one row or column wide
    c, plan, trips = _fp32(2, 16, 32, 72, 40, 1)
    assert plan == (2, 2, 8, 8) and c.cin % 64 == 8 and c.cout < 64                        # second ci tile of 8 channels, padded co rows
    c, plan, trips = _fp32(4, 24, 48, 256, 256, 1)
    assert plan == (3, 3, 36, 16) and sorted(set(trips)) == [2, 3] and trips.count(3) == 4   # the double buffer wraps; has_next false mid-run
    c, plan, trips = _fp32(2, 8, 16, 320, 16, 1)
    assert plan == (1, 1, 2, 2) and -(-c.cin // 64) == 5 and 64 - c.cout == 48
    c, plan, trips = _fp32(1, 2, 2, 8, 8, 2)
    assert plan == (1, 1, 1, 1) and wr.out_hw(c.H, c.W, 2) == (1, 1)
    c, plan, trips = _fp32(2, 18, 34, 64, 64, 2)
    Ho, Wo = wr.out_hw(c.H, c.W, 2)
    assert (Ho, Wo) == (9, 17) and plan == (3, 3, 18, 18) and Ho % 4 == 1 and Wo % 8 == 1
    assert 2 * (Ho - 1) + 1 < c.H and 2 * (Wo - 1) + 1 < c.W                               # the last pixel's bottom / right tap is inside the map
    c, plan, trips = _fp32(3, 16, 16, 128, 64, 2)
    assert plan == (2, 1, 6, 6) and set(trips) == {1} and -(-c.cin // 64) == 2
    c, plan, trips = _fp32(3, 32, 32, 256, 256, 2)
    assert plan == (4, 2, 24, 16) and sorted(set(trips)) == [1, 2] and trips.count(2) == 8   # several tiles per workgroup at stride 2
    # the table as a whole: both strides run more than one trip, and the one-trip form
    for s in (1, 2):
        assert any(max(wr.trips_fp32(*k[:6])) > 1 for k in wr.FP32_CASES if k.stride == s)


def _bf16(*shape):
    i = wr.index_of('bf16', *shape)
    return wr.BF16_CASES[i], wr.plan_bf16(*shape), wr.stages_bf16(*shape)


def test_bf16_cases_reach_the_paths_they_name():
    assert len({tuple(c[:6]) for c in wr.BF16_CASES}) == len(wr.BF16_CASES) and all(c.why for c in wr.BF16_CASES)
    c, plan, st = _bf16(1, 1, 8, 8, 8, 1)
    assert plan == (1, 1, 4, 1) and st == [1] and c.H < wr.stage_rows_bf16(1) and c.W < wr.WG_DW
    c, plan, st = _bf16(1, 5, 32, 64, 64, 1)
    assert plan == (1, 1, 8, 1) and st == [2] and c.W == wr.WG_DW and c.H == wr.stage_rows_bf16(1) + 1
    c, plan, st = _bf16(1, 16, 33, 64, 64, 1)
    assert plan == (2, 2, 8, 4) and st == [2, 2] and c.W - wr.WG_DW == 1                   # second strip of one column; rows 7 | 8 split
    c, plan, st = _bf16(2, 12, 31, 72, 40, 1)
    assert plan == (1, 2, 8, 4) and st == [2, 1] and c.W == wr.WG_DW - 1 and c.cin % 64 == 8 and c.cout == 40
    c, plan, st = _bf16(1, 40, 64, 64, 64, 1)
    assert plan == (2, 5, 8, 10) and st == [2] * 5
    c, plan, st = _bf16(1, 40, 24, 704, 640, 1)
    assert plan == (1, 2, 20, 2) and st == [5, 5]
    assert min(st) + 1 > wr.ring_groups_bf16(1) and min(st) > wr.ring_groups_bf16(1) - 1     # x groups 0 .. n_st and dy stages wrap
    c, plan, st = _bf16(1, 8, 32, 320, 16, 1)
    assert plan == (1, 1, 8, 1) and st == [2] and -(-c.cin // 64) == 5
    c, plan, st = _bf16(1, 2, 2, 8, 8, 2)
    assert plan == (1, 1, 2, 1) and st == [1] and wr.out_hw(c.H, c.W, 2) == (1, 1)
    c, plan, st = _bf16(2, 18, 66, 64, 64, 2)
    assert wr.out_hw(c.H, c.W, 2) == (9, 33) and plan == (2, 3, 4, 12) and st == [2, 2, 1]   # odd rows against TR = 2; strip of one column
    c, plan, st = _bf16(1, 32, 64, 128, 64, 2)
    assert plan == (1, 4, 4, 4) and st == [2] * 4
    c, plan, st = _bf16(1, 32, 48, 704, 640, 2)
    assert plan == (1, 2, 8, 2) and st == [4, 4] and min(st) + 1 > wr.ring_groups_bf16(2)
    for s in (1, 2):
        assert any(wr.plan_bf16(*k[:6])[1] >= 2 for k in wr.BF16_CASES if k.stride == s)
        assert any(wr.plan_bf16(*k[:6])[0] >= 2 for k in wr.BF16_CASES if k.stride == s)


def test_largest_case_is_the_one_with_the_largest_workspace():
    c = wr.FP32_CASES[wr.largest('fp32')]
    assert tuple(c[:6]) == (4, 24, 48, 256, 256, 1)                                        # 16 splits x 16 pairs x 9 x 64 x 64 floats = 37.7 MB
    c = wr.BF16_CASES[wr.largest('bf16')]
    assert (c.cin, c.cout) == (704, 640) and wr.plan_bf16(*c[:6])[3] * 110 * 9 * 4096 * 4 > (1 << 20)


# ---- the tolerance and the exact test can see a real fault ------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,i', CASES)
def test_one_lost_pixel_changes_an_integer_and_one_lost_row_leaves_the_bound(kind, i):
    c = wr.TABLES[kind][i]
    d = wr.case_data(kind, i, True)
    dy = d['dy'].copy()
    dy[-1, -1, -1, :] = 0                                                                  # the last output pixel, dropped
    assert (wr.wgrad3x3(d['x'], dy, c.stride)[0] != d['dw'])[:, :, 1, 1].all()             # its centre tap is always inside the map
    f = wr.case_data(kind, i, False)
    dy = f['dy'].copy()
    dy[-1, -1, :, :] = 0                                                                   # the last output row of the last frame
    lost = np.abs(wr.wgrad3x3(f['x'], dy, c.stride)[0] - f['dw'])[:, :, 1, 1]
    assert (lost > 2 * wr.bound(f['S'], f['K'])[:, :, 1, 1]).mean() > 0.5
