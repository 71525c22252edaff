"""The reference, patterns and case table of tests/sparse_conv_refs.py, checked on the CPU: the reference against torch's float64 conv2d on
the scattered canvas, the integer variants against the condition that makes bit-equality owed, tile_tap_counts against a pixel-by-pixel
walk, the table against the list of branch points of k_sparse_conv_s2 it has to reach (conditions on the table, not on the kernel), the
points against the pillariser's fp32 cell arithmetic, and the weight pack against its stated layout.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_conv_refs as sr
from pcp_amd import pack

ALL = list(range(len(sr.CASES)))
IDS = [c.name for c in sr.CASES]

ROW_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)     # chunk edges, the row-tile edge, both ends
ITEM_COUNTS = (0, 1, 2, 3, 4, 5, 6, 7, 36)                                    # every residue of the four-item loop and its tails; the full table


@functools.lru_cache(maxsize=None)
def _counts(i):
    return sr.tile_tap_counts(sr.occupancy(sr.CASES[i]))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', ALL, ids=IDS)
def test_reference_equals_torch_float64_conv2d_on_the_canvas(i):
    c = sr.CASES[i]
    ho, wo = sr.out_hw(c.ny, c.nx, 2)
    for variant in ('ints', 'float'):
        d = sr.case_data(i, variant)
        canvas = torch.from_numpy(sr.canvas_of(d['occ'], d['coords'], d['pf'])).permute(0, 3, 1, 2)
        want = F.conv2d(canvas, torch.from_numpy(d['w'].astype(np.float64)), torch.from_numpy(d['b'].astype(np.float64)), stride=2,
                        padding=1).permute(0, 2, 3, 1).numpy()
        assert d['pre'].shape == want.shape == (c.B, ho, wo, c.cout)
        assert (np.abs(d['pre'] - want) <= 1e-12 * d['S']).all()
        assert (d['S'] >= np.abs(d['pre'])).all() and (d['S'] > 0).all()
        if variant == 'ints':
            assert np.array_equal(d['pre'], want) and d['bar'] is None
            assert np.array_equal(d['pre'].astype(np.float32).astype(np.float64), d['pre'])         # the fp32 cast loses nothing
        else:
            assert d['bar'].shape == want.shape and (d['bar'] > 0).all()
        assert (d['pre'] < 0).any() and (d['pre'] > 0).any()                                        # the ReLU has something to clamp
        # an empty pixel holds the bias alone
        quiet = _counts(i).pixel_taps == 0
        assert np.array_equal(d['pre'][quiet], np.broadcast_to(d['b'].astype(np.float64), d['pre'][quiet].shape))


def test_reference_refuses_a_pillar_list_that_is_not_the_occupancy():
    d = sr.case_data(sr.CASE_INDEX['odd_density_05'], 'ints')
    coords = np.array(d['coords'])
    sr.reference(d['occ'], coords[::-1], d['pf'], d['w'], d['b'], False)                            # any order of the same set is a pillar list
    with pytest.raises(AssertionError):
        sr.reference(d['occ'], coords[1:], d['pf'], d['w'], d['b'], False)
    moved = coords.copy()
    moved[0, 2:] = moved[1, 2:]
    moved[0, 0] = moved[1, 0]
    with pytest.raises(AssertionError):
        sr.reference(d['occ'], moved, d['pf'], d['w'], d['b'], False)


def test_one_hot_weights_turn_the_reference_into_a_lookup():
    """the lookup of one_hot_expect (no sum in it) and the convolution with one_hot_weights agree, tap by tap, on a non-square grid"""
    d = sr.case_data(sr.CASE_INDEX['wide_density_05_005'], 'float')
    for tap in range(9):
        y, _S = sr.reference(d['occ'], d['coords'], d['pf'], sr.one_hot_weights(tap), np.zeros(64, np.float32), False)
        assert np.array_equal(y, sr.one_hot_expect(d['occ'], d['coords'], d['pf'], tap).astype(np.float64)) and y.any()


# ---- the integer variants --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', ALL, ids=IDS)
def test_integer_cases_meet_the_condition_that_makes_bit_equality_owed(i):
    for cout in {sr.CASES[i].cout} | (set(sr.COUTS) if sr.CASES[i].name == sr.COUT_CASE else set()):
        d = sr.case_data(i, 'ints', cout)
        for a in (d['pf'], d['w'], d['b']):
            assert (a == np.round(a)).all() and (a.size == 0 or (np.abs(a).min() >= 1 and np.abs(a).max() <= 8))
        assert d['S'].max() < sr.EXACT and d['S'].max() <= 9 * 64 * 64 + 8


def test_bf16_cases_hold_sums_that_are_no_bf16_values():
    """integers above 256 in magnitude, odd ones among them (exact ties between 256 and 512), on both sides of 0"""
    for name in sr.BF16_CASES:
        pre = sr.case_data(sr.CASE_INDEX[name], 'ints')['pre']
        for sign in (1, -1):
            v = pre * sign
            assert (v > 256).any() and ((v > 256) & (v < 512) & (v % 2 == 1)).any()


# ---- the geometry ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['wide_density_05_005', 'tall_density_05', 'odd_full', 'two_columns_density_05', 'one_cell'])
def test_tile_tap_counts_equal_a_walk_over_pixels_and_taps(name):
    occ = sr.occupancy(sr.CASES[sr.CASE_INDEX[name]])
    B, ny, nx = occ.shape
    ho, wo = (ny - 1) // 2 + 1, (nx - 1) // 2 + 1
    t = sr.tile_tap_counts(occ)
    count, lo, hi, taps = np.zeros_like(t.count), np.zeros_like(t.lo), np.zeros_like(t.hi), np.zeros_like(t.pixel_taps)
    for b in range(B):
        for oy in range(ho):
            for ox in range(wo):
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
                        if 0 <= iy < ny and 0 <= ix < nx and occ[b, iy, ix]:
                            count[b, oy // 8, ox // 16, ky * 3 + kx] += 1
                            (lo if (oy % 8) * 16 + ox % 16 < 64 else hi)[b, oy // 8, ox // 16, ky * 3 + kx] += 1
                            taps[b, oy, ox] += 1
    assert np.array_equal(t.count, count) and np.array_equal(t.lo, lo) and np.array_equal(t.hi, hi) and np.array_equal(t.pixel_taps, taps)
    assert np.array_equal(t.items, ((count + 31) // 32).sum(-1)) and t.items.max() <= 36 and count.max() <= 128


def test_every_occupied_cell_is_read_as_its_parity_class_says():
    """(even, even) once, the mixed classes twice, (odd, odd) four times, less only at the far edges of the map"""
    for py, px, reads in ((0, 0, 1), (1, 0, 2), (0, 1, 2), (1, 1, 4)):
        occ = np.zeros((1, 32, 64), bool)
        occ[0, 10 + py, 20 + px] = True
        t = sr.tile_tap_counts(occ)
        assert t.count.sum() == reads and t.pixel_taps.max() == 1


def test_first_k_of_class_places_exactly_k_rows():
    for tile, k in (((1, 1), 1), ((0, 1), 33), ((1, 0), 128)):
        t = sr.tile_tap_counts(sr._occ(sr.first_k_of_class(tile, sr.EE, k), 1, 32, 64))
        want = np.zeros_like(t.count)
        want[0, tile[0], tile[1], 4] = k
        assert np.array_equal(t.count, want)
    t = sr.tile_tap_counts(sr._occ(sr.first_k_of_class((0, 0), sr.EO, 65), 1, 20, 36))
    assert t.count[0, 0, 0].tolist() == [0, 0, 0, 61, 0, 65, 0, 0, 0] and t.items[0, 0, 0] == 5


def test_the_table_reaches_every_branch_point_of_the_kernel():
    counts, items = set(), set()
    hi_only = lo_only = nine = one = False
    for i in ALL:
        t = _counts(i)
        counts |= set(t.count.ravel().tolist())
        items |= set(t.items.ravel().tolist())
        hi_only |= bool(((t.lo == 0) & (t.hi > 0)).any())
        lo_only |= bool(((t.hi == 0) & (t.lo > 0)).any())
        nine |= bool((t.pixel_taps == 9).any())
        one |= bool((t.pixel_taps == 1).any())
    assert not [n for n in ROW_COUNTS if n not in counts], sorted(counts)
    assert not [n for n in ITEM_COUNTS if n not in items], sorted(items)
    assert hi_only and lo_only and nine and one


def test_the_named_cases_place_what_their_names_say():
    """the branch points are placed on purpose: the cases named after a count hold it, whatever the random ones add"""
    def tap4(name):
        return sorted(set(_counts(sr.CASE_INDEX[name]).count[..., 4].ravel().tolist()) - {0})
    assert tap4('wide_edge_tile_15_16') == [15, 16] and tap4('tall_17_31_33') == [17, 31, 33] and tap4('whole_1_32_128') == [1, 32, 128]
    assert tap4('whole_63_64_65') == [63, 64, 65] and tap4('whole_96_97_127') == [96, 97, 127]
    assert _counts(sr.CASE_INDEX['wide_items_5_6_7']).items[:, 0, 0].tolist() == [5, 6, 7]
    assert (_counts(sr.CASE_INDEX['whole_full']).items == 36).all() and _counts(sr.CASE_INDEX['whole_full']).count.max() == 128
    assert 127 in _counts(sr.CASE_INDEX['whole_full_but_one']).count[..., 4]
    t = _counts(sr.CASE_INDEX['whole_wave1_only'])
    assert (t.lo == 0).all() and t.hi.any()
    t = _counts(sr.CASE_INDEX['whole_wave0_only'])
    assert (t.hi == 0).all() and t.lo.any()
    # the last cell row and column of the odd grid are read through the centre tap of the last pixel row and column
    t = _counts(sr.CASE_INDEX['odd_last_row_and_column'])
    assert t.pixel_taps[0, 8].any() and t.pixel_taps[0, :, 16].any()


def test_the_table_holds_the_grid_shapes_that_tell_x_from_y():
    cs = sr.CASES
    assert any(c.nx > c.ny for c in cs) and any(c.nx < c.ny for c in cs) and any(c.nx % 2 for c in cs) and any(c.ny % 2 for c in cs)
    assert any(((c.nx - 1) // 2 + 1) % 16 for c in cs) and any(((c.ny - 1) // 2 + 1) % 8 for c in cs)
    shapes = {(c.nx, c.ny) for c in cs}
    assert shapes == {(36, 20), (20, 36), (33, 17), (64, 32), (1, 1), (2, 31)}
    assert {c.B for c in cs} == {1, 2, 3} and max(c.B * c.nx * c.ny for c in cs) <= 3 * 64 * 32
    # different occupancy in each frame at the same cells
    assert any(c.B > 1 and (sr.occupancy(c)[0] != sr.occupancy(c)[1]).any() for c in cs)
    for name in (sr.COUT_CASE, sr.WIDE_ROW_CASE, sr.OTHER_PILLARISER_CASE) + sr.ONE_HOT_CASES + sr.BF16_CASES:
        assert name in sr.CASE_INDEX
    assert {(sr.CASES[sr.CASE_INDEX[n]].nx, sr.CASES[sr.CASE_INDEX[n]].ny) for n in sr.ONE_HOT_CASES} == {(36, 20), (20, 36), (33, 17)}


# ---- the points ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', ALL, ids=IDS)
def test_points_land_in_exactly_the_occupied_cells(i):
    c = sr.CASES[i]
    occ, g = sr.occupancy(c), sr.grid_of(c)
    pts = sr.points_for(occ, g)
    assert pts.dtype == np.float32 and pts.shape[1] == 5 and occ.sum() <= pts.shape[0] <= 3 * occ.sum()
    assert np.array_equal(sr.cells_of_points(pts, g), occ)
    # centres are exact: (i + 0.5) / 4 in float64 is the float32 value
    assert np.array_equal(pts[:, 1:3].astype(np.float64) * 4 - 0.5, np.round(pts[:, 1:3].astype(np.float64) * 4 - 0.5))
    assert (pts[:, 3] > sr.Z_RANGE[0]).all() and (pts[:, 3] < sr.Z_RANGE[1]).all()
    coords = sr.coords_of(occ)
    assert coords.shape == (occ.sum(), 4) and occ[coords[:, 0], coords[:, 2], coords[:, 3]].all()
    key = (coords[:, 0].astype(np.int64) * c.nx + coords[:, 3]) * c.ny + coords[:, 2]               # the merged cell id, ascending
    assert (np.diff(key) > 0).all()


# ---- the pack --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cout', sr.COUTS)
def test_pack_lays_the_taps_out_as_the_header_states(cout):
    """[9 (ky * 3 + kx)][64][64 (cin)], rows from cout on zero, the bias padded to 64 with zeros"""
    _pf, w, b = sr.inputs(0, 'ints', 0, cout)
    wp, bp = pack.pack_conv3x3_sparse_s2(torch.from_numpy(np.array(w)), torch.from_numpy(np.array(b)))
    wp, bp = wp.numpy(), bp.numpy()
    assert wp.shape == (9, 64, 64) and wp.dtype == np.float32 and bp.shape == (64,)
    for t in range(9):
        assert np.array_equal(wp[t, :cout], w[:, :, t // 3, t % 3])
    assert not wp[:, cout:].any() and np.array_equal(bp[:cout], b) and not bp[cout:].any()
