"""The references, scales, input generators and case tables of tests/conv3x3_refs.py, checked on the CPU: the references against torch's
float64 conv2d, the integer variants against the conditions that make bit-equality owed, pack.py's filter transforms of the integer
weights against exactness in fp32, an fp32 emulation of both Winograd pipelines against the references (exact on the integer cases in two
summation orders, inside the T bar on the float cases), planted mistakes in that emulation against both kinds of case, and every case
against the entry points' argument checks.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3x3_refs as cr
from pcp_amd import pack

ALL_CASES = [(t, i) for t in cr.TABLES for i in range(len(cr.TABLES[t]))]
M_OF = {'f2': 2, 'f4': 4}
# the ragged case of each Winograd family the planted mistakes run on: (table, index)
PLANT_CASES = {2: ('wino2', 1), 4: ('wino4_fused', 1)}


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _m(table):
    return M_OF[cr.TABLE_ALGO[table]]


# ---- the references --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i', ALL_CASES)
def test_references_equal_torch_float64_conv2d(table, i):
    c = cr.TABLES[table][i]
    for variant in ('ints', 'float'):
        d = cr.case_data(table, i, variant)
        want = F.conv2d(_nchw(d['x']), _t(d['w']), _t(d['b']), stride=c.stride, padding=1).permute(0, 2, 3, 1).numpy()
        assert d['pre'].shape == want.shape == (c.B,) + cr.out_hw(c.H, c.W, c.stride) + (c.cout,)
        if variant == 'ints':
            assert np.array_equal(d['pre'], want) and np.abs(d['pre']).max() > 0
            assert np.array_equal(d['pre'].astype(np.float32).astype(np.float64), d['pre'])         # the fp32 cast loses nothing
            assert d['bar'] is None
        else:
            assert (np.abs(d['pre'] - want) <= 1e-12 * d['S']).all()
            assert (d['bar'] > 0).all() and d['bar'].shape == want.shape
        assert (d['S'] >= np.abs(d['pre'])).all()
        assert (d['pre'] < 0).any() and (d['pre'] > 0).any()                                        # the ReLU has something to clamp


def test_winograd_scale_bounds_the_result_and_shrinks_where_the_patch_is_padding():
    """T >= |y| (the triangle inequality through the transforms), and T at one position of a border tile is below T at the same position
    of an interior tile of the same constant map"""
    for m in (2, 4):
        x, w, b = cr.uniform(900, 1, (2, 9, 11, 8)), cr.uniform(900, 2, (12, 8, 3, 3)), cr.uniform(900, 3, (12,))
        y, _S = cr.conv3x3(x, w, b, 1, False)
        T = cr.wino_scale(x, w, b, m)
        assert T.shape == y.shape and (T >= np.abs(y)).all()
        ones, wo = np.ones((1, 3 * m, 3 * m, 8), np.float32), np.abs(w)
        T1 = cr.wino_scale(ones, wo, np.zeros(12), m)
        assert (T1[0, 0, 0] < T1[0, m, m]).all() and (T1[0, -1, -1] < T1[0, 2 * m - 1, 2 * m - 1]).all()


# ---- the integer variants --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i', ALL_CASES)
def test_integer_cases_meet_the_condition_that_makes_bit_equality_owed(table, i):
    d = cr.case_data(table, i, 'ints')
    algo = cr.TABLE_ALGO[table]
    x, w, b = d['x'], d['w'], d['b']
    if algo in ('direct', 'bf16x3'):
        for a in (x, w):
            assert (a == np.round(a)).all() and np.abs(a).min() >= 1 and np.abs(a).max() <= 8
        assert (b == np.round(b)).all() and d['S'].max() < cr.EXACT_DIRECT
        bits = np.ascontiguousarray(x).view(np.uint32)
        assert not (bits & np.uint32(0xFFFF)).any()                                                 # exact bf16: the low split terms are 0
    else:
        top = 1 if x.shape[-1] > 384 else 2
        assert set(np.unique(x)) <= set(range(-top, top + 1)) and set(np.unique(w)) <= {-9.0, 0.0, 9.0}
        assert 0.4 < (x != 0).mean() < 0.6 and (0.4 < (w != 0).mean() < 0.6 or x.shape[-1] > 384)
        assert (4 * b == np.round(4 * b)).all() and (b != np.round(b)).any() and (b != 0).all()
        partial, transform = cr.wino_headroom(x, w, _m(table))
        print('%s[%d]: partial sums %.3f * 2^24, output transform %.3f * 2^24 (units of 2^-6)' % (table, i, partial / 2 ** 24, transform / 2 ** 24))
        assert partial < cr.EXACT_WINO and transform < cr.EXACT_WINO


def test_dense_small_integers_do_not_fit_the_winograd_condition():
    """why the Winograd tables have their own generator: dense [-8, 8] data at 64 input channels leaves the exact range"""
    x, w = cr.ints8(950, 1, (1, 8, 8, 64)), cr.ints8(950, 3, (16, 64, 3, 3))
    assert max(cr.wino_headroom(x, w, 4)) > cr.EXACT_WINO


@pytest.mark.parametrize('table,i', cr.WINO_CASES)
def test_packed_filter_transform_of_the_integer_weights_is_exact(table, i):
    """the U pack.py makes from the 9 k weights, read back from the packed layouts: wherever the exact G g G^T is not 0 it is that value, a
    multiple of 2^-6 (F(4x4)) / 2^-2 (F(2x2)), and the U of the references; where the exact value is 0 it is 0 for F(2x2) and 0 or a residue
    of pack.py's float64 sum for F(4x4), and all residues together stay below 2^-31 in every intermediate (conv3x3_refs' docstring)"""
    c = cr.TABLES[table][i]
    d = cr.case_data(table, i, 'ints')
    m = _m(table)
    wt, bt = torch.from_numpy(np.array(d['w'])), torch.from_numpy(np.array(d['b']))
    if table == 'wino2':
        p, _b, cpad = pack.pack_conv3x3_winograd(wt, bt)                                            # [cin/8][16][cout_pad][8]
        u = p.permute(2, 0, 3, 1).reshape(cpad, c.cin, 4, 4)
    elif table == 'wino2_ws':
        p, _b, cpad = pack.pack_conv3x3_winograd_ws(wt, bt)
        u = pack.unpack_winograd_ws(p, cpad)
    elif table == 'wino4':
        p, _b, cpad = pack.pack_conv3x3_winograd4(wt, bt)                                           # [36][cout_pad][cin]
        u = p.permute(1, 2, 0).reshape(cpad, c.cin, 6, 6)
    else:
        p, _b, cpad = pack.pack_conv3x3_winograd4f(wt, bt)                                          # [cin/8][36][cout_pad][8]
        u = p.permute(2, 0, 3, 1).reshape(cpad, c.cin, 6, 6)
        for repack, other in ((pack.repack_winograd4f_to_4h, pack.pack_conv3x3_winograd4h), (pack.repack_winograd4f_to_4c, pack.pack_conv3x3_winograd4c)):
            q = other(wt, bt)[0]
            assert torch.equal(q, repack(p)) and torch.equal(q.flatten().sort().values, p.flatten().sort().values)   # pure permutations
    u = u.numpy()
    unit = 64.0 if m == 4 else 4.0
    G = cr.WINO[m][2]
    exact = np.einsum('ia,ncab,jb->ncij', G, cr.f64(d['w']), G) * unit                              # integers, up to float64's rounding of 1/6
    assert np.abs(np.round(exact) - exact).max() < 1e-9
    exact = np.round(exact) / unit
    assert np.array_equal(cr.wino_u(d['w'], m).astype(np.float64), exact) and not u[c.cout:].any()
    live = exact != 0
    assert np.array_equal(u[:c.cout][live].astype(np.float64), exact[live])
    residue = np.abs(u[:c.cout][~live])
    assert residue.max() <= 2.0 ** -50 and (m == 4 or not residue.any())
    _partial, _transform, added = cr.wino_headroom(d['x'], d['w'], m, u_packed=u[:c.cout])
    print('%s[%d]: %d residues of %d zeros, largest %.3g; at most %.3g in any intermediate' % (table, i, (residue != 0).sum(), residue.size, residue.max(), added))
    assert added < 2.0 ** -31


# ---- the fp32 emulation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i', cr.WINO_CASES)
def test_fp32_emulation_is_exact_on_integer_cases_and_inside_the_bar_on_float_cases(table, i):
    m = _m(table)
    d = cr.case_data(table, i, 'ints')
    want = d['pre'].astype(np.float32)
    for reverse in (False, True):
        assert np.array_equal(cr.wino_emulate(d['x'], d['w'], d['b'], m, reverse=reverse), want)
    d = cr.case_data(table, i, 'float')
    worst = 0.0
    for reverse in (False, True):
        err = np.abs(cr.f64(cr.wino_emulate(d['x'], d['w'], d['b'], m, reverse=reverse)) - d['pre'])
        worst = max(worst, float((err / d['bar']).max()))
    print('%s[%d]: largest err / bar of the emulation %.3f' % (table, i, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('plant', cr.PLANTS)
@pytest.mark.parametrize('m', [2, 4])
def test_planted_mistakes_change_an_integer_case_and_exceed_the_bar_of_a_float_case(m, plant):
    table, i = PLANT_CASES[m]
    c = cr.TABLES[table][i]
    assert c.H % m and c.W % m and c.cin > 8                                                        # the last tile IS ragged; skipping a slice leaves some
    d = cr.case_data(table, i, 'ints')
    got = cr.wino_emulate(d['x'], d['w'], d['b'], m, plant=plant)
    wrong = got != d['pre'].astype(np.float32)
    assert wrong.any()
    if plant == 'drop_tap':                                                                         # only the last tile, and not all of the map
        assert not wrong[:, :(c.H - 1) // m * m, :, :].any() and not wrong[:, :, :(c.W - 1) // m * m, :].any() and not wrong[:-1].any()
    if plant == 'border':                                                                           # only pixels next to the map's edge
        assert not wrong[:, 1:c.H - 1, 1:c.W - 1, :].any()
    d = cr.case_data(table, i, 'float')
    err = np.abs(cr.f64(cr.wino_emulate(d['x'], d['w'], d['b'], m, plant=plant)) - d['pre'])
    assert (err > d['bar']).any()


def test_a_reduced_precision_product_exceeds_the_float_bars_at_the_smallest_cin():
    """what the float cases are for: operands rounded to bf16 (8 significand bits) before the products leave the bar of every family at
    its smallest input-channel count, while the integer cases cannot see it (their values are exact in bf16)"""
    from wgrad3x3_refs import bf16_round
    for table, i in (('direct_s1', 0), ('wino2', 0), ('wino4', 0), ('wino4_fused', 0), ('bf16x3_s1', 0)):
        c = cr.TABLES[table][i]
        assert c.cin == min(k.cin for k in cr.TABLES[table])
        d = cr.case_data(table, i, 'float')
        low, _S = cr.conv3x3(bf16_round(d['x']), bf16_round(d['w']), d['b'], c.stride, False)
        assert (np.abs(low - d['pre']) > d['bar']).mean() > 0.5
        d = cr.case_data(table, i, 'ints')
        if cr.TABLE_ALGO[table] in ('direct', 'bf16x3'):
            assert np.array_equal(bf16_round(d['x']), d['x']) and np.array_equal(bf16_round(d['w']), d['w'])


# ---- the tables ------------------------------------------------------------------------------------------------------------------------

def test_every_case_meets_its_kernels_argument_checks_and_every_kernel_has_a_window_case():
    need = {'direct_s1': (16, 1), 'direct_s2': (16, 1), 'wino2': (8, 1), 'wino2_ws': (32, 1), 'wino4': (32, 4), 'wino4_fused': (8, 4),
            'bf16x3_s1': (16, 1), 'bf16x3_s2': (16, 1)}
    assert set(need) == set(cr.TABLES) == set(cr.TABLE_ALGO)
    for table, cases in cr.TABLES.items():
        kmod, nmod = need[table]
        for c in cases:
            assert c.cin % kmod == 0 and c.cout % nmod == 0 and c.why
            assert c.stride == (2 if table.endswith('_s2') else 1)
        assert min(c.cin for c in cases) == kmod                                                    # the smallest cin the kernel takes
    assert set(cr.WINDOW_CASE) == set(cr.KERNELS)
    for name, i in cr.WINDOW_CASE.items():
        c = cr.TABLES[cr.KERNELS[name].table][i]
        assert (c.cin + cr.PAD_IN) % 4 == 0 and (c.cout + cr.PAD_OUT) % 4 == 0 and cr.OFF_IN % 4 == 0 and cr.OFF_OUT % 4 == 0   # 16-byte aligned
        assert c.cin > 16 and (c.H % 16 or c.W % 16)
    c = cr.TABLES['bf16x3_s1'][2]                                                                   # the 32-row form's launch rule, restated
    assert c.B * -(-c.H // 32) * -(-c.W // 16) * (-(-c.cout // 64)) >= 512
    for c in cr.TABLES['bf16x3_s1'][:2]:
        assert c.B * -(-c.H // 32) * -(-c.W // 16) * (-(-c.cout // 64)) < 512
