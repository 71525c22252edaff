"""The float64 references, the pack decoder, the input generators and the case tables of tests/mp_forward_refs.py, checked on the CPU:
the references against torch's float64 convolutions, the integer and tie variants against the condition that makes bit-equality owed
(max S < 2^22), the one-hot expectations against the references, and every case against the entry points' documented preconditions
(restated from include/pcp_hip_mp.h, not read from the kernels).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mp_forward_refs as mr

CONV = [(t, i) for t in ('fast', 'gen') for i in range(len(mr.CONV_TABLES[t]))]
EXACT = 2.0 ** 22


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _close(a, b, scale):
    return np.allclose(a, b, rtol=1e-12, atol=1e-12 * float(np.max(scale)))


# ---- the references --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stride,relu,shape', [(1, False, (2, 7, 9, 5, 6)), (2, False, (2, 7, 9, 5, 6)), (2, True, (1, 5, 5, 3, 4)),
                                               (1, True, (1, 1, 1, 3, 2))])
def test_conv_reference_equals_torch_float64(stride, relu, shape):
    B, H, W, cin, cout = shape
    x, w, b = mr.uniform(801, 1, (B, H, W, cin)), mr.uniform(801, 2, (cout, cin, 3, 3)), mr.uniform(801, 3, (cout,))
    y, S = mr.conv3x3(x, w, b, stride, relu)
    want = F.conv2d(_nchw(x), _t(w), _t(b), stride=stride, padding=1)
    want = (want.clamp_min(0) if relu else want).permute(0, 2, 3, 1).numpy()
    assert y.shape == want.shape == (B,) + mr.out_hw(H, W, stride) + (cout,)
    assert _close(y, want, S)
    S_want = F.conv2d(_nchw(np.abs(x)), _t(np.abs(w)), _t(np.abs(b)), stride=stride, padding=1).permute(0, 2, 3, 1).numpy()
    assert np.allclose(S, S_want, rtol=1e-12, atol=0) and (S >= np.abs(y)).all()
    if relu and y.size > 16:
        assert (y == 0).any() and (y > 0).any()


def test_dgrad_reference_equals_conv_transpose2d_and_is_not_the_forward_of_the_same_weights():
    B, H, W, cin, cout = 2, 6, 7, 5, 4
    dy, w = mr.uniform(802, 1, (B, H, W, cout)), mr.uniform(802, 2, (cout, cin, 3, 3))
    dx, S = mr.conv3x3_dgrad(dy, w)
    want = F.conv_transpose2d(_nchw(dy), _t(w), stride=1, padding=1).permute(0, 2, 3, 1).numpy()
    assert dx.shape == (B, H, W, cin) and _close(dx, want, S)
    assert np.allclose(S, mr.conv3x3_dgrad(np.abs(dy), np.abs(w))[0], rtol=1e-12, atol=0)
    # the flip matters: the forward conv on the merely transposed weights is something else
    unflipped = mr.conv3x3(dy, w.transpose(1, 0, 2, 3), np.zeros(cin), 1, False)[0]
    assert float(np.abs(unflipped - dx).max()) > 0.1
    flipped = mr.conv3x3(dy, w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1], np.zeros(cin), 1, False)[0]
    assert _close(dx, flipped, S)


def test_taps_inside_counts_the_taps_of_border_pixels():
    n = mr.taps_inside(5, 7, 1)
    assert n.shape == (5, 7) and n[0, 0] == 4 and n[0, 3] == 6 and n[2, 3] == 9 and n[4, 6] == 4
    n = mr.taps_inside(5, 6, 2)                                            # odd H: the last row's bottom halo is outside; even W: inside
    assert n.shape == (3, 3) and n[0, 0] == 4 and n[2, 2] == 6 and n[1, 1] == 9 and n[2, 0] == 4
    assert mr.taps_inside(1, 1, 1).tolist() == [[1]]


# ---- the packs -------------------------------------------------------------------------------------------------------------------------

def _pack_by_the_header(v, contraction, out_pad):
    """[contraction / 16][out_pad / 64][9][2][64][8], one element at a time from the logical (out, contraction, ky, kx) array"""
    flat = np.zeros((contraction // 16) * (out_pad // 64) * 9 * 2 * 64 * 8, v.dtype)
    for o in range(v.shape[0]):
        for k in range(contraction):
            for tap in range(9):
                at = (((((k // 16) * (out_pad // 64) + o // 64) * 9 + tap) * 2 + (k % 16) // 8) * 64 + o % 64) * 8 + k % 8
                flat[at] = v[o, k, tap // 3, tap % 3]
    return flat


def test_unpack_inverts_a_pack_built_from_the_layout_description():
    out, K, out_pad = 72, 48, 128
    v = mr.uniform(803, 1, (out, K, 3, 3))
    got = mr.unpack3x3(_pack_by_the_header(v, K, out_pad), K, out_pad)
    assert got.shape == (out_pad, K, 3, 3) and np.array_equal(got[:out], v) and not got[out:].any()


def test_pack_expect_rounds_ties_to_even_once_and_places_the_transposed_form():
    w = np.zeros((16, 16, 3, 3), np.float32)
    w[0, 1, 0, 2], w[2, 3, 2, 1], w[4, 5, 1, 1] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)
    v = mr.pack_expect(w, None, False)
    assert v[0, 1, 0, 2] == 1.0 and v[2, 3, 2, 1] == 1 + 2.0 ** -6 and v[4, 5, 1, 1] == -1.0 and np.count_nonzero(v) == 3
    t = mr.pack_expect(w, None, True)                                      # (out, contraction) = (cin, cout), tap 8 - t
    assert t[1, 0, 2, 0] == 1.0 and t[3, 2, 0, 1] == 1 + 2.0 ** -6 and t[5, 4, 1, 1] == -1.0 and np.count_nonzero(t) == 3
    fold = np.ones(16, np.float32)
    fold[0], fold[2] = 0.5, 3.0                                            # fold indexes the weight's first axis in both forms
    assert mr.pack_expect(w, fold, False)[0, 1, 0, 2] == 0.5 and mr.pack_expect(w, fold, True)[1, 0, 2, 0] == 0.5
    # 3 * (1 + 3 * 2^-8) = 3.03515625, between the bf16 neighbours 3.03125 and 3.046875: one rounding of the fp32 product gives
    # 3.03125; rounding w first (1.015625) and then the product 3.046875 would not
    assert mr.pack_expect(w, fold, False)[2, 3, 2, 1] == 3.03125
    assert mr.bf16_round(np.float32(3.0) * mr.bf16_round(w)[2, 3, 2, 1])[0] == 3.046875


def test_tie_generators_make_exact_ties():
    x = mr.tie_ints(804, 1, (4096,))
    k = np.abs(x) - 0.5
    assert x.dtype == np.float32 and np.array_equal(k, np.floor(k)) and k.min() == 128 and k.max() == 255
    r = np.abs(mr.bf16_round(x))
    assert (np.abs(r - np.abs(x)) == 0.5).all() and (r % 2 == 0).all() and (r > np.abs(x)).any() and (r < np.abs(x)).any()
    w = mr.tie_weights(804, 3, (4096,))
    r = mr.bf16_round(w)
    m, e = np.frexp(np.abs(w))                                             # |w| = m 2^e, m in [0.5, 1): the bf16 grid there has spacing 2^-8
    assert (np.abs(np.abs(r) - np.abs(w)) == np.ldexp(2.0 ** -9, e)).all() and len(np.unique(e)) == 5
    assert torch.equal(torch.from_numpy(r), torch.from_numpy(w).bfloat16().float())
    bits = mr.bf16_bits(r)
    assert (bits & 1 == 0).all()                                           # nearest EVEN
    f = mr.tie_fold(804, 5, 64)
    assert (np.log2(f[::2]) % 1 == 0).all() and (np.log2(f[1::2]) % 1 != 0).all()
    i8 = mr.ints8(804, 7, (4096,))
    assert (i8 != 0).all() and np.abs(i8).max() == 8 and np.array_equal(i8, np.round(i8)) and len(np.unique(i8)) == 16


def test_pw_pack_equals_the_project_pack_where_that_pads_to_64():
    from pcp_amd import pack
    for kind, shape, f in (('plain', (72, 96), pack.pack_plain), ('s2d', (72, 32, 2, 2), pack.pack_conv2x2_s2),
                           ('d2s', (32, 72, 2, 2), pack.pack_convT2x2_s2)):
        w, b = mr.uniform(805, 1, shape), mr.uniform(805, 2, (72,))
        wp, bp, cp = f(torch.from_numpy(w), torch.from_numpy(b))
        got_w, got_b = mr.pw_pack(kind, w, b, cp)
        assert cp == 128 and np.array_equal(got_w, wp.numpy()) and np.array_equal(got_b, bp.numpy())
    w8, b8 = mr.pw_pack('plain', np.ones((8, 32), np.float32), np.ones(8, np.float32), 64)
    assert w8.shape == (2, 64, 16) and w8[:, :8].all() and not w8[:, 8:].any() and b8.tolist() == [1.0] * 8 + [0.0] * 56


# ---- exactness: what makes bit-equality owed ---------------------------------------------------------------------------------------------

def _exact_case(d, what):
    assert float(d['S'].max()) < EXACT, what
    y = d['y']
    assert np.array_equal(y, np.round(y)) and np.array_equal(y.astype(np.float32).astype(np.float64), y), what


@pytest.mark.parametrize('table,i', CONV + [('mis', 0)])
def test_integer_conv_cases_make_every_partial_sum_exact(table, i):
    c = mr.MISALIGNED if table == 'mis' else mr.CONV_TABLES[table][i]
    forms = [False, True] if c.stride == 1 else [False]
    for dgrad in forms:
        d = mr.conv_data(table, i, 'ints', dgrad)
        for a in (d['x'], d['w']):
            assert a.dtype == np.float32 and (a != 0).all() and np.abs(a).max() <= mr.INT_MAX and np.array_equal(mr.bf16_round(a), a)
        assert np.array_equal(d['b'], np.round(d['b'])) and np.abs(d['b']).max() <= mr.INT_MAX
        _exact_case(d, (table, i, dgrad))
    if 'f32' in c.ins:
        d = mr.conv_data(table, i, 'ties')
        assert not np.array_equal(mr.bf16_round(d['x']), d['x'])
        _exact_case(d, (table, i, 'ties'))
        # truncation while staging (k instead of the even neighbour) changes nearly every output element the ReLU does not clamp either way
        trunc = (np.trunc(np.abs(d['x'])) * np.sign(d['x'])).astype(np.float32)
        other = mr.conv3x3(trunc, d['w'], d['b'], c.stride, d['relu'])[0]
        assert ((other != d['y']) | (d['y'] == 0)).mean() > 0.9 and (other != d['y']).mean() > 0.4
    assert c.B * c.H * c.W <= (18432 if tuple(c[:5]) == (32, 256, 6, 48, 64) else 16384)


@pytest.mark.parametrize('i', range(len(mr.PW_CASES)))
def test_integer_pointwise_cases_make_every_partial_sum_exact(i):
    for variant in ('ints', 'ties'):
        d = mr.pw_data(i, variant)
        _exact_case(d, (i, variant))
        assert d['y'].shape == mr.pw_out_shape(mr.PW_CASES[i])


@pytest.mark.parametrize('i', range(len(mr.PWG_CASES)))
def test_integer_pointwise_wgrad_cases_make_every_partial_sum_exact(i):
    d = mr.pwg_data(i, True)
    assert float(d['S'].max()) < EXACT and np.array_equal(d['out'], np.round(d['out']))
    # accumulate=1 onto integer contents: the old value is one more term of the sum
    old = mr.pwg_old(i)
    assert old.shape == d['out'].shape and np.array_equal(old, np.round(old)) and (old != 0).all()
    assert float((np.abs(mr.f64(old)) + d['S']).max()) < EXACT


@pytest.mark.parametrize('side', ['a', 'b'])
def test_integer_lattice_wgrad_operands_make_every_partial_sum_exact(side):
    d = mr.lattice_data(side)
    n, k, B, gh, gw = mr.WGRAD_LATTICE
    assert d['rows'] == B * gh * gw and d['big'].shape[:3] == (B, 2 * gh, 2 * gw) and len(d['taps']) == 4
    for a in (d['big'], d['small']):
        assert (a != 0).all() and np.abs(a).max() <= mr.INT_MAX and np.array_equal(a, np.round(a))
    for (_gh, _gw, ky, kx), out, S in d['taps']:
        assert out.shape == (n, k) and float(S.max()) < EXACT and np.array_equal(out, np.round(out))
    assert len({out.tobytes() for _lat, out, _S in d['taps']}) == 4      # the four taps differ: one in another's place shows


def test_the_chosen_biases_put_exact_ties_of_the_bf16_store_into_the_integer_cases():
    """odd integers between 256 and 512 in magnitude lie midway between two bf16 values; tie_bias makes two per case where the sums are
    large enough, each with a non-zero bias on its channel"""
    n_cases = 0
    for table, i in CONV:
        d = mr.conv_data(table, i, 'ints')
        flat = d['y'].reshape(-1, d['y'].shape[-1])
        for p, n in d['ties']:
            v = flat[p, n]
            assert 256 < abs(v) < 512 and v % 2 == 1 and d['b'][n] != 0
            r = float(mr.bf16_round(np.float32(v))[0])
            assert abs(r - v) == 1 and (r / 2) % 2 == 0                  # the even neighbour on the grid of spacing 2
        n_cases += len(d['ties']) == 2
        if not d['relu'] and len(d['ties']) == 2:
            assert flat[d['ties'][0]] > 0 > flat[d['ties'][1]]
    assert n_cases >= 12                                                   # every case with cin >= 32 and more than a pixel
    assert sum(len(mr.pw_data(i, 'ints')['ties']) == 2 for i in range(len(mr.PW_CASES))) >= 3
    # bias after the rounding, or a truncating store, misses them
    d = mr.conv_data('fast', 1, 'ints')
    p, n = d['ties'][0]
    v = d['y'].reshape(-1, d['y'].shape[-1])[p, n]
    late = float(mr.bf16_round(np.float32(v - d['b'][n]))[0]) + d['b'][n]
    assert late != float(mr.bf16_round(np.float32(v))[0])


def test_float_variants_are_exact_in_bf16_and_cached_read_only():
    d = mr.conv_data('fast', 2, 'float')
    for a in (d['x'], d['w']):
        assert torch.equal(torch.from_numpy(np.array(a)).bfloat16().float(), torch.from_numpy(np.array(a)))
    assert mr.conv_data('fast', 2, 'float') is d and d['K'].max() == 9 * 96 + 1 and d['K'].min() == 4 * 96 + 1
    with pytest.raises(ValueError):
        d['x'][0, 0, 0, 0] = 1.0


# ---- the one-hot helpers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i,dgrad', mr.PLACE_CASES)
def test_one_hot_expectation_equals_the_reference(table, i, dgrad):
    c = mr.CONV_TABLES[table][i]
    w, picks = mr.one_hot_conv(50 + i, c.cin, c.cout, dgrad)
    assert w.sum() == c.cout and {(ky, kx) for ky, kx, _c in picks} == {(a, b) for a in range(3) for b in range(3)}
    assert w.shape == ((c.cin, c.cout, 3, 3) if dgrad else (c.cout, c.cin, 3, 3))
    x = mr.place_map(60 + i, (c.B, c.H, c.W, c.cin))
    assert (x != 0).all()
    want = mr.one_hot_conv_expect(x, picks, c.stride, dgrad)
    ref = mr.conv3x3_dgrad(x, w)[0] if dgrad else mr.conv3x3(x, w, np.zeros(c.cout), c.stride, False)[0]
    assert np.array_equal(ref, want)
    # channel 0 takes tap (0, 0): forward it reads the pixel up-left, so row 0 and column 0 are exactly 0; the data gradient reads
    # down-right, so the LAST row and column are
    assert picks[0][:2] == (0, 0)
    if dgrad:
        assert not want[:, -1, :, 0].any() and not want[:, :, -1, 0].any() and want[:, 0, 0, 0].all()
        assert np.array_equal(want[:, :-1, :-1, 0], x[:, 1:, 1:, picks[0][2]])
    else:
        assert not want[:, 0, :, 0].any() and not want[:, :, 0, 0].any()
        if c.stride == 1:
            assert np.array_equal(want[:, 1:, 1:, 0], x[:, :-1, :-1, picks[0][2]])
    # channel 8 takes tap (2, 2): at stride 2 on an odd map the last output row reads below the map
    if c.stride == 2 and c.H % 2 == 1:
        assert not want[:, -1, :, 8].any() and not want[:, :, -1, 8].any() and want[:, 0, 0, 8].all()


# ---- the tables against the documented preconditions and the paths they name --------------------------------------------------------------

@pytest.mark.parametrize('table,i', CONV + [('mis', 0)])
def test_conv_cases_meet_the_preconditions_of_pcp_mp_conv3x3(table, i):
    c = mr.MISALIGNED if table == 'mis' else mr.CONV_TABLES[table][i]
    assert c.why and c.cin % 16 == 0 and c.stride in (1, 2) and c.cin % 4 == 0 and c.cout % 4 == 0
    assert set(c.ins) <= {'bf16', 'f32'} and set(c.outs) <= {'bf16', 'f32'} and c.ins and c.outs
    if table == 'fast':
        assert mr.fast_plan(c) and c.ins == mr.BF                          # stride 1, bf16 in, cin % 32 == 0, cout_pad <= 512
        assert 'bf16' not in c.outs or c.cout % 8 == 0                     # bf16 out of the fast kernel
        assert c.th in (0, 8, 16) and mr.tile_rows(c, 1) == 16 and mr.tile_rows(c, mr.TH8_MIN) == 8
        assert c.th != 0 or mr.tile_rows(c) == 8                           # left to the rule, every case gets 8-row items
    if table == 'gen':
        assert c.th == 0
        for ins in c.ins:                                                  # bf16 input reaches the general kernel only through stride 2 or cin % 32 == 16
            assert ins == 'f32' or c.stride == 2 or c.cin % mr.MC_CK == 16


def test_conv_tables_hold_the_cases_and_reach_the_paths_they_name():
    shapes = {t: [tuple(c[:6]) for c in mr.CONV_TABLES[t]] for t in mr.CONV_TABLES}
    assert shapes['fast'][:7] == [(32, 64, 1, 8, 32, 1), (64, 64, 1, 9, 33, 1), (96, 72, 2, 7, 31, 1), (64, 132, 1, 16, 40, 1),
                                  (384, 64, 1, 8, 32, 1), (64, 512, 1, 8, 32, 1), (64, 64, 3, 17, 70, 1)]
    assert shapes['fast'][7:10] == [(64, 64, 1, 17, 33, 1), (64, 128, 2, 33, 31, 1), (128, 64, 1, 16, 32, 1)]
    assert {s[:5] for s in shapes['gen']} == {(16, 64, 1, 1, 1), (16, 64, 1, 19, 23), (48, 64, 1, 17, 17), (64, 64, 2, 16, 32),
                                              (64, 128, 2, 15, 33), (32, 40, 2, 9, 9)}
    F = mr.FAST_CASES
    assert F[0].cin // mr.MC_CK == 1 and mr.conv_items(F[0], 8) == 1
    assert F[1].H % 8 == 1 and F[1].W % mr.MC_TW == 1
    assert (F[2].cin // mr.MC_CK) % 2 == 1 and F[2].cout % 64 == 8
    assert F[3].cout % 8 == 4 and F[3].outs == mr.F32 and -(-F[3].cout // 64) == 3
    assert F[4].cin // mr.MC_CK == 12 and F[5].cout == mr.MC_MAX_COUT
    assert mr.conv_items(F[6], 8) == 27 and F[6].H % 8 == 1 and F[6].W % mr.MC_TW == 6 and mr.run_steps(F[6], 8) == set()
    many = F[10]
    items = mr.conv_items(many, 8)
    assert items == 288 > mr.CUS and mr.tile_rows(many) == 8 and many.cin == mr.MC_CK and many.B * many.H * many.W <= 18432
    assert items - mr.CUS == 32 and mr.run_steps(many, 8) == {'nb'}        # 32 workgroups with two items: channel blocks of one tile
    assert [c.th for c in F[7:10]] == [16, 16, 16] and all(mr.run_steps(c, 16) == set() for c in F[7:10])


def _runs_by_the_rule(c, th):
    """the runs a second time, item by item: workgroup l of nwg walks per (+ 1 for the first rem) consecutive items"""
    n = c.B * ((c.H + th - 1) // th) * ((c.W + 31) // 32) * ((c.cout + 63) // 64)
    nwg = min(n, 256)
    owner, it = [], 0
    for wg in range(nwg):
        for _ in range(n // nwg + (1 if wg < n % nwg else 0)):
            owner.append(wg)
            it += 1
    assert it == n
    return owner


@pytest.mark.parametrize('i,th', [(11, 8), (12, 16)])
def test_multi_item_cases_step_tile_column_tile_row_and_frame_inside_a_run(i, th):
    """the persistent kernel decodes its first item and then ADVANCES counters (channel block fastest, tile column, tile row, frame) for
    the item it copies and, one stage behind, for the item it computes: these cases make some workgroup take every carry, with two
    slices per item so that the copy of the next item's first slice runs under the current item's last"""
    c = mr.FAST_CASES[i]
    assert c.th == th and c.cin // mr.MC_CK == 2 and c.B * c.H * c.W <= 16384
    assert -(-c.W // mr.MC_TW) >= 2 and -(-c.H // th) >= 2 and -(-c.cout // mr.MC_BN) >= 2 and c.B >= 2
    runs = mr.fast_runs(c, th)
    owner = _runs_by_the_rule(c, th)
    assert len(runs) == mr.CUS and [wg for wg, (b, e) in enumerate(runs) for _ in range(b, e)] == owner
    assert max(e - b for b, e in runs) == 3 and min(e - b for b, e in runs) == 2
    assert mr.run_steps(c, th) == {'nb', 'tx', 'ty', 'frame'}
    # and from the decode itself: inside some run the tile column steps, it wraps with a tile-row step, and both wrap into the next frame
    seen = set()
    for b, e in runs:
        for it in range(b, e - 1):
            (f0, y0, x0, n0), (f1, y1, x1, n1) = mr.item_coords(c, th, it), mr.item_coords(c, th, it + 1)
            if n1 == 0 and n0 == c.cout // 64 - 1:
                seen.add((f1 - f0, y1 - y0, x1 - x0))
    assert seen == {(0, 0, 1), (0, 1, -1), (1, -1, -1)}
    assert mr.item_coords(c, th, mr.conv_items(c, th) - 1) == (c.B - 1, 1, 1, c.cout // 64 - 1)
    G = mr.GEN_CASES
    assert G[4].H % 2 == 1 and G[4].W % 2 == 1 and G[3].H % 2 == 0 and G[3].W % 2 == 0
    assert G[2].cin % 32 == 16 and G[2].ins == mr.BF and G[2].H % mr.MG_TW == 1
    m = mr.MISALIGNED
    assert mr.fast_plan(m) and m.cout % 8 == 0
    for t, i in mr.WINDOW_CASES:
        assert mr.CONV_TABLES[t][i].outs == mr.BOTH
    assert {t for t, _i in mr.WINDOW_CASES} == {'fast', 'gen'}


def test_pointwise_cases_meet_the_preconditions_and_hold_the_sizes_asked_for():
    P = mr.PW_CASES
    for c in P:
        assert c.why and c.cin % 32 == 0 and c.cout % 8 == 0
        if c.kind == 's2d':
            assert c.H % 2 == 0 and c.W % 2 == 0
    assert [c.B for c in P if c.kind == 'plain'] == [1, 127, 128, 129, 385]
    assert {c.cin for c in P} == {32, 96, 512} and {c.cout for c in P} == {8, 64, 72}
    assert {(c.B, c.H, c.W) for c in P if c.kind == 's2d'} >= {(1, 2, 2), (2, 6, 10), (1, 16, 18)}
    assert {(c.B, c.H, c.W) for c in P if c.kind == 'd2s'} == {(1, 1, 1), (3, 5, 7), (1, 8, 17)}
    split = [c for c in P if c.kind == 's2d' and c.B * (c.H // 2) * (c.W // 2) > mr.MPW_BM]
    assert split and all(mr.MPW_BM % (c.W // 2) != 0 for c in split)       # the block boundary falls inside a row
    W = mr.PWG_CASES
    assert all(c.n % 8 == 0 and c.k % 8 == 0 for c in W) and {(72, 40, 377), (64, 64, 1)} <= {tuple(c[:3]) for c in W}
    assert [tuple(c[:3]) for c in W[:-1]] == [tuple(c[:3]) for c in mr.WGRAD_CASES if c.n % 8 == 0 and c.k % 8 == 0] and all(c.why for c in W)
    ring = W[-1]
    assert ring.rows % mr.MWG_ROWS == 1 and mr.pwg_split(ring.rows, ring.n, ring.k) == (6, 1) and 6 > mr.MWG_NST
    # the split plan of the bf16 kernel (32-row stages), as the reasons state it
    split = {tuple(c[:3]): mr.pwg_split(c.rows, c.n, c.k) for c in W}
    assert split[(72, 40, 377)] == (12, 1) and 377 - 11 * 32 == 25
    assert split[(64, 64, 127)] == (4, 1) and split[(64, 64, 128)] == (4, 1) and split[(64, 64, 129)] == (5, 1) and split[(64, 64, 1)] == (1, 1)
    assert split[(256, 256, 1000)] == (32, 4)
    assert split[(256, 256, 8229)] == (258, 32) and 258 == 32 * 8 + 2 and 8229 - 257 * 32 == 5
    n, k, _B, _gh, _gw = mr.WGRAD_LATTICE
    assert n % 8 == 0 and k % 8 == 0
