"""The forward kernels of the bf16 training loop -- pcp_mp_conv3x3 (k_mp_conv3x3_s1, k_mp_conv3x3_gen; forward and data-gradient weight
forms), the packers pcp_mp_pack_conv3x3 / _group, pcp_mp_pointwise (three modes) and pcp_mp_pointwise_wgrad -- against the float64
references and the case tables of tests/mp_forward_refs.py.  Integer inputs: bit-equality with the float64 result, for a bf16 output with
its round-to-nearest-even.  Tie inputs: where the fp32 -> bf16 roundings happen.  One-hot weights: placement, element by element.  Float
inputs: 2 * bound(S, K) of tests/pointwise_refs.py, element by element, on the bf16-rounded operands; for a bf16 output
bf16_round(want - tol) <= got <= bf16_round(want + tol), both ends clamped where a ReLU follows.  Each bound comparison prints the largest
|got - ref| / (2 * bound) it saw (pytest -s).  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import mp_forward_refs as mr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.678                # what every element a launch must not write holds before it (rounded to the buffer's type)
POISON = 1e30                    # what every element a launch must not READ holds
OK, ARG, UNSUPPORTED = 0, 1, 4   # PCP_OK, PCP_ERR_ARG, PCP_ERR_UNSUPPORTED of include/pcp_hip.h


def _mods():
    from pcp_amd import lib, ops, train_ops
    return lib, ops, train_ops


def _dt(s):
    return torch.bfloat16 if s == 'bf16' else torch.float32


def _dev(a, s='f32'):
    """float32 host array -> contiguous device tensor of storage type s"""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).to(_dt(s)).contiguous()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().double().numpy()


def _pad64(n):
    return (n + 63) // 64 * 64


def _owed(want, outs):
    """what an output of storage type outs owes for the exact float64 result"""
    return want if outs == 'f32' else mr.f64(mr.bf16_round(want.astype(np.float32)))


def _exactly(got, want, outs, what):
    g = _host(got)
    want = _owed(want, outs)
    assert g.shape == want.shape, (g.shape, want.shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    bad = g != want
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        where = np.argwhere(bad)
        raise AssertionError('%s: %d of %d elements differ, largest difference %g; first at %s: got %r, want %r; channels hit: %s%s'
                             % (what, int(bad.sum()), bad.size, float(np.abs(g - want).max()), at, g[at], want[at],
                                sorted({int(a[-1]) for a in where})[:12],
                                '; columns hit: %s' % sorted({int(a[2]) for a in where})[:12] if g.ndim == 4 else ''))


def _within(got, d, outs, what, factor=2):
    """factor * bound(S, K) around the value before the ReLU, both ends rounded to the output's type, then clamped"""
    g = _host(got)
    assert g.shape == d['pre'].shape, (g.shape, d['pre'].shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    tol = factor * mr.bound(d['S'], d['K'])
    lo, hi = _owed(d['pre'] - tol, outs), _owed(d['pre'] + tol, outs)
    if d['relu']:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    bad = int(((g < lo) | (g > hi)).sum())
    if outs == 'f32':
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(tol > 0, np.abs(g - d['y']) / tol, 0.0)
        worst = 'max |got - ref| / (%d * bound) = %.5f' % (factor, float(ratio.max()))
    else:                                                                    # the store's rounding dwarfs the bound: count instead
        worst = '%d of %d elements are not the rounded reference itself' % (int((g != _owed(d['y'], outs)).sum()), g.size)
    print('\nRATIO %-60s %s' % (what, worst))
    assert bad == 0, '%s: %d of %d elements outside the bound; %s' % (what, bad, g.size, worst)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _wide(inner, ld, off, fill):
    """`inner` (..., c) at channels [off, off + c) of a (..., ld) buffer of the same type that holds `fill` everywhere else"""
    buf = torch.full(tuple(inner.shape[:-1]) + (ld,), fill, dtype=inner.dtype, device=DEV)
    buf[..., off:off + inner.shape[-1]] = inner
    return buf


def _untouched_outside(buf, off, c):
    """every element of `buf` outside channels [off, off + c) still holds the bits of SENT in the buffer's type"""
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[off:off + c] = False
    sent = _bits(torch.full((1,), SENT, dtype=buf.dtype)).item()
    assert sent != 0
    return bool((_bits(buf)[..., keep] == sent).all())


def _name(c, ins, outs):
    if isinstance(c, mr.Conv):
        return 'conv (%d,%d,%d) %d->%d s%d %s->%s' % (c.B, c.H, c.W, c.cin, c.cout, c.stride, ins, outs)
    return '%s (%d,%d,%d) %d->%d %s->%s' % (c.kind, c.B, c.H, c.W, c.cin, c.cout, ins, outs)


# ---- running a conv case -------------------------------------------------------------------------------------------------------------------

def _case(table, i):
    return mr.MISALIGNED if table == 'mis' else mr.CONV_TABLES[table][i]


def _combos(tables, stride1_only=False, ins_only=None):
    out = []
    for t in tables:
        for i, c in enumerate(mr.CONV_TABLES[t]):
            if stride1_only and c.stride != 1:
                continue
            out += [(t, i, a, b) for a in c.ins for b in c.outs if ins_only in (None, a)]
    return out


ALL = _combos(('fast', 'gen'))
STRIDE1 = _combos(('fast', 'gen'), stride1_only=True)
F32_IN = _combos(('gen',), ins_only='f32')


def _pack3(w, transpose=False, fold=None):
    tops = _mods()[2]
    return tops.mp_pack_conv3x3(_dev(w), transpose, fold_scale=None if fold is None else _dev(fold))


def _bias(b, opad):
    bp = torch.zeros(opad, dtype=torch.float32, device=DEV)
    bp[:len(b)] = _dev(b)
    return bp


def _desc(c, ins, outs, ld_in=None, ld_out=None, relu=0):
    lib = _mods()[0]
    return lib.MpConv3x3(c.B, c.H, c.W, c.cin, c.cout, _pad64(c.cout), c.stride, ld_in or c.cin, ld_out or c.cout, relu,
                         lib.DT_BF16 if ins == 'bf16' else lib.DT_F32, lib.DT_BF16 if outs == 'bf16' else lib.DT_F32)


def _plan(c, ins, outs, **kw):
    """(fast_kernel, executed_flops) of pcp_mp_conv3x3_plan.  The plan sees the descriptor, not the pointers"""
    lib = _mods()[0]
    fast, flops = ctypes.c_int32(-1), ctypes.c_double(0.0)
    d = _desc(c, ins, outs, **kw)
    assert lib.load().pcp_mp_conv3x3_plan(ctypes.byref(d), ctypes.byref(fast), ctypes.byref(flops)) == OK
    return fast.value, flops.value


def _setup(c, table, ins, outs, lib_option):
    """the item size the case asks for, and the plan's word on which kernel and which item size the case reaches"""
    if c.th:
        lib_option('mp_th16_min', 1 if c.th == 16 else mr.TH8_MIN)
    fast, flops = _plan(c, ins, outs)
    assert fast == (1 if table == 'fast' else 0)
    if table == 'fast':
        th = c.th or 8
        px = c.B * (-(-c.H // th) * th) * (-(-c.W // mr.MC_TW) * mr.MC_TW)
        assert flops == 2.0 * px * _pad64(c.cout) * 9.0 * c.cin            # padded to th-row items: the option took


def _conv(c, d, ins, outs, dgrad=False, x=None, out=None, in_ch_off=0, out_ch_off=0, w=None, b=None, relu=None):
    tops = _mods()[2]
    packed, opad = _pack3(d['w'] if w is None else w, dgrad)
    assert opad == _pad64(c.cout)
    x = _dev(d['x'], ins) if x is None else x
    return tops.mp_conv3x3(x, packed, _bias(d['b'] if b is None else b, opad), c.cin, c.cout, opad, stride=c.stride,
                           relu=d['relu'] if relu is None else relu, out=out, out_dtype=_dt(outs), in_ch_off=in_ch_off, out_ch_off=out_ch_off)


# ---- a. integer inputs, bit for bit --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i,ins,outs', ALL)
def test_conv_integer_inputs_give_the_float64_result_bit_for_bit(table, i, ins, outs, lib_option):
    """every product and partial sum is an integer below 2^24 (asserted on the CPU): any order owes the exact result, and a bf16 output
    its nearest-even rounding -- sums above 256 are no bf16 values, and the bias puts two exact ties into every case large enough"""
    c, d = _case(table, i), mr.conv_data(table, i, 'ints')
    _setup(c, table, ins, outs, lib_option)
    _exactly(_conv(c, d, ins, outs), d['y'], outs, _name(c, ins, outs))


@pytest.mark.parametrize('table,i,ins,outs', STRIDE1)
def test_conv_data_gradient_form_gives_the_scattered_gradient_bit_for_bit(table, i, ins, outs, lib_option):
    """the transpose pack of the (cin, cout, 3, 3) weights of a conv with the kernel's channel counts swapped, against the scatter
    reference: a tap that is not flipped, or channels that are not swapped, change integers"""
    c, d = _case(table, i), mr.conv_data(table, i, 'ints', True)
    _setup(c, table, ins, outs, lib_option)
    _exactly(_conv(c, d, ins, outs, dgrad=True), d['y'], outs, _name(c, ins, outs) + ' data gradient')


def test_an_8_byte_aligned_bf16_window_takes_the_general_kernel():
    """in_ch_off 4 of a bf16 buffer: the pointer is 8 but not 16 bytes aligned, which the direct-to-LDS kernel cannot copy from.  The
    plan sees only the descriptor and names the fast kernel; what ran is not asserted, the result is"""
    c, d = mr.MISALIGNED, mr.conv_data('mis', 0, 'ints')
    ld = c.cin + 8
    for outs in c.outs:
        assert _plan(c, 'bf16', outs, ld_in=ld)[0] == 1
        xw = _wide(_dev(d['x'], 'bf16'), ld, 4, POISON)
        assert (xw.data_ptr() + 2 * 4) % 16 == 8
        _exactly(_conv(c, d, 'bf16', outs, x=xw, in_ch_off=4), d['y'], outs, _name(c, 'bf16', outs) + ' at in_ch_off 4')


# ---- b. where the roundings are ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i,ins,outs', F32_IN)
def test_general_kernel_rounds_its_fp32_input_to_nearest_even_while_staging(table, i, ins, outs):
    """fp32 maps of +-(k + 0.5), k in [128, 255]: every element is an exact tie of the bf16 rounding.  Nearest-even gives the even
    neighbour, truncation k, half-away k + 1: the reference on bf16_round(x) is owed bit for bit, and the other two differ from it in
    nearly every element (asserted on the CPU)"""
    c, d = _case(table, i), mr.conv_data(table, i, 'ties')
    _exactly(_conv(c, d, 'f32', outs), d['y'], outs, _name(c, 'f32', outs) + ' tie inputs')


PACK_SHAPES = [(80, 48), (64, 32), (16, 16)]                                # (cout, cin): both forms pad (128 / 64), one has none, the smallest


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('transpose', [False, True])
def test_packer_rounds_the_fp32_product_once_to_nearest_even(transpose, fold):
    """tie weights (exact ties of the bf16 grid), with and without fold_scale (powers of two keep the ties, the other entries make the
    fp32 product round before the bf16 rounding): the decoded device pack equals pack_expect bit for bit, and the rows between the
    output channels and out_pad are exact zeros"""
    for n, (cout, cin) in enumerate(PACK_SHAPES):
        w = mr.tie_weights(5000 + n, 1, (cout, cin, 3, 3))
        f = mr.tie_fold(5000 + n, 5, cout) if fold else None
        K, O = (cout, cin) if transpose else (cin, cout)
        packed, opad = _pack3(w, transpose, f)
        assert opad == _pad64(O) and packed.dtype == torch.bfloat16 and packed.numel() == (K // 16) * (opad // 64) * 9 * 2 * 64 * 8
        torch.cuda.synchronize()
        got = mr.unpack3x3(packed.view(torch.int16).cpu().numpy().view(np.uint16), K, opad)
        want = mr.bf16_bits(mr.pack_expect(w, f, transpose))
        assert want.shape == (O, K, 3, 3)
        bad = got[:O] != want
        assert not bad.any(), 'pack (%d, %d) transpose %d fold %d: %d of %d values differ, first at [out, k, ky, kx] = %s' % (
            cout, cin, transpose, fold, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]))
        assert not got[O:].any()                                             # +0.0, bit for bit


def test_grouped_pack_writes_the_bytes_of_the_single_packs():
    """three jobs of different sizes, both forms, tie weights, in one launch: the bytes of per-layer pcp_mp_pack_conv3x3 calls"""
    _lib, _ops, tops = _mods()
    grp = tops.MpPackGroup()
    owner = torch.nn.Identity()
    single = {}
    for n, (cout, cin) in enumerate(PACK_SHAPES):
        w = _dev(mr.tie_weights(5100 + n, 1, (cout, cin, 3, 3)))
        for tr in (False, True):
            ref, opad = tops.mp_pack_conv3x3(w, tr)
            single[(n, tr)] = ref
            grp.add((n, tr), owner, w, tr, torch.full_like(ref, 7.0), opad)
    grp.run(torch.device(DEV))
    torch.cuda.synchronize()
    assert len(grp.jobs) == 6
    for key, (_o, _j, (_w, dst)) in grp.jobs.items():
        assert _same_bits(dst, single[key]), key


# ---- c. placement, exact -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('outs', ['bf16', 'f32'])
@pytest.mark.parametrize('table,i,dgrad', mr.PLACE_CASES)
def test_one_hot_weights_copy_the_shifted_map_bit_for_bit(table, i, dgrad, outs, lib_option):
    """output channel n copies channel c of the pixel one tap away (tap n % 9; the opposite shift in the data-gradient form) of a map of
    arbitrary bf16 values: a sum of one value and zeros, exact in either output type, and exactly 0 where the tap leaves the map, at all
    four borders.  A wrong tap, channel, halo or swizzle column shows at the element"""
    c = _case(table, i)
    ins = c.ins[0]
    _setup(c, table, ins, outs, lib_option)
    w, picks = mr.one_hot_conv(50 + i, c.cin, c.cout, dgrad)
    x = mr.place_map(60 + i, (c.B, c.H, c.W, c.cin))
    want = mr.one_hot_conv_expect(x, picks, c.stride, dgrad)
    got = _conv(c, None, ins, outs, dgrad=dgrad, x=_dev(x, ins), w=w, b=np.zeros(c.cout, np.float32), relu=False)
    _exactly(got, want, 'f32', _name(c, ins, outs) + (' one-hot, data gradient' if dgrad else ' one-hot'))      # bf16 values: nothing to round


# ---- d. float inputs against the bound -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table,i,ins,outs', ALL)
def test_conv_float_inputs_within_the_bound(table, i, ins, outs, lib_option):
    c, d = _case(table, i), mr.conv_data(table, i, 'float')
    _setup(c, table, ins, outs, lib_option)
    _within(_conv(c, d, ins, outs), d, outs, _name(c, ins, outs))


# ---- channel windows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('outs', ['bf16', 'f32'])
@pytest.mark.parametrize('table,i', mr.WINDOW_CASES)
def test_conv_channel_windows_of_wider_buffers(table, i, outs):
    """the input is a window of a wider buffer that holds 1e30 elsewhere (one read outside the window -- a halo column taken from the
    neighbouring row's record, a chunk past the last channel -- swamps the integers), the output a window of a wider buffer whose other
    elements must keep the sentinel's bits"""
    c, d = _case(table, i), mr.conv_data(table, i, 'ints')
    ins = c.ins[-1]
    assert _plan(c, ins, outs, ld_in=c.cin + 24, ld_out=c.cout + 24)[0] == (1 if table == 'fast' else 0)
    xw = _wide(_dev(d['x'], ins), c.cin + 24, 8, POISON)
    Ho, Wo = mr.out_hw(c.H, c.W, c.stride)
    out = torch.full((c.B, Ho, Wo, c.cout + 24), SENT, dtype=_dt(outs), device=DEV)
    _conv(c, d, ins, outs, x=xw, out=out, in_ch_off=8, out_ch_off=8)
    _exactly(out[..., 8:8 + c.cout], d['y'], outs, _name(c, ins, outs) + ' windows')
    assert _untouched_outside(out, 8, c.cout)


# ---- the pointwise family ----------------------------------------------------------------------------------------------------------------

PW = [(i, a, b) for i in range(len(mr.PW_CASES)) for a in ('bf16', 'f32') for b in ('bf16', 'f32')]


def _pw(c, d, ins, outs, x=None, out=None, in_ch_off=0, out_ch_off=0, w=None, b=None, relu=None):
    lib, _ops, tops = _mods()
    cp = _pad64(c.cout)
    wp, bp = mr.pw_pack(c.kind, d['w'] if w is None else w, d['b'] if b is None else b, cp)
    mode = {'plain': lib.PW_PLAIN, 's2d': lib.PW_SPACE2DEPTH, 'd2s': lib.PW_DEPTH2SPACE}[c.kind]
    x = _dev(d['x'], ins) if x is None else x
    return tops.mp_pointwise(x, _dev(wp, 'bf16'), _dev(bp), mode, c.cin, c.cout, cp, relu=c.relu if relu is None else relu, out=out,
                             in_ch_off=in_ch_off, out_ch_off=out_ch_off, out_dtype=_dt(outs))


@pytest.mark.parametrize('i,ins,outs', PW)
def test_pointwise_integer_inputs_give_the_float64_result_bit_for_bit(i, ins, outs):
    c, d = mr.PW_CASES[i], mr.pw_data(i, 'ints')
    _exactly(_pw(c, d, ins, outs), d['y'], outs, _name(c, ins, outs))


@pytest.mark.parametrize('i,outs', [(i, o) for i in range(len(mr.PW_CASES)) for o in ('bf16', 'f32')])
def test_pointwise_rounds_its_fp32_input_to_nearest_even_while_staging(i, outs):
    c, d = mr.PW_CASES[i], mr.pw_data(i, 'ties')
    _exactly(_pw(c, d, 'f32', outs), d['y'], outs, _name(c, 'f32', outs) + ' tie inputs')


@pytest.mark.parametrize('i,ins,outs', PW)
def test_pointwise_float_inputs_within_the_bound(i, ins, outs):
    c, d = mr.PW_CASES[i], mr.pw_data(i, 'float')
    _within(_pw(c, d, ins, outs), d, outs, _name(c, ins, outs))


@pytest.mark.parametrize('outs', ['bf16', 'f32'])
@pytest.mark.parametrize('kind', ['plain', 's2d', 'd2s'])
def test_pointwise_selection_weights_copy_the_selected_channels_bit_for_bit(kind, outs):
    """0/1 weights on a map of arbitrary bf16 values: plain copies one channel per output channel, space-to-depth one (tap, channel) of the
    2x2 block, depth-to-space a different channel permutation per tap"""
    if kind == 'plain':
        c = mr.Pw('plain', 131, 0, 0, 96, 72, False, 'every output channel copies one input channel')
        w, pick = mr.selection_plain(1, c.cout, c.cin)
        x = mr.place_map(71, (c.B, c.cin))
        want = mr.f64(x)[:, pick]
        assert np.array_equal(mr.plain(x, w, np.zeros(c.cout))[0], want)
    elif kind == 's2d':
        c = mr.Pw('s2d', 3, 6, 10, 32, 72, False, 'every output channel copies one (tap, channel) of its 2x2 block')
        _sel, pick = mr.selection_plain(2, c.cout, 4 * c.cin)              # pick = tap * cin + channel
        assert len({int(p) // c.cin for p in pick}) == 4
        w = np.zeros((c.cout, c.cin, 2, 2), np.float32)
        for n, p in enumerate(pick):
            w[n, p % c.cin, (p // c.cin) >> 1, (p // c.cin) & 1] = 1.0
        x = mr.place_map(72, (c.B, c.H, c.W, c.cin))
        want = np.stack([mr.f64(x)[:, (p // c.cin) >> 1::2, (p // c.cin) & 1::2, p % c.cin] for p in pick], -1)
        assert np.array_equal(mr.space2depth(x, w, np.zeros(c.cout))[0], want)
    else:
        c = mr.Pw('d2s', 3, 5, 7, 96, 72, False, 'every tap has its own channel permutation')
        w = np.zeros((c.cin, c.cout, 2, 2), np.float32)
        x = mr.place_map(73, (c.B, c.H, c.W, c.cin))
        want = np.empty((c.B, 2 * c.H, 2 * c.W, c.cout), np.float64)
        picks = []
        for tap in range(4):
            sel, pick = mr.selection_plain(10 + tap, c.cout, c.cin)
            w[:, :, tap >> 1, tap & 1] = sel.T
            want[:, (tap >> 1)::2, (tap & 1)::2, :] = mr.f64(x)[..., pick]
            picks.append(tuple(pick))
        assert len(set(picks)) == 4 and np.array_equal(mr.depth2space(x, w, np.zeros(c.cout))[0], want)
    got = _pw(c, None, 'bf16', outs, x=_dev(x, 'bf16'), w=w, b=np.zeros(c.cout, np.float32))
    _exactly(got, want, 'f32', _name(c, 'bf16', outs) + ' selection')


PW_WINDOWS = [1, 8, 10]                                                     # plain 127 x 96 -> 72, s2d 144 rows, d2s 105 rows


@pytest.mark.parametrize('i,ins,outs', [(i, a, b) for i in PW_WINDOWS for a in ('bf16', 'f32') for b in ('bf16', 'f32')])
def test_pointwise_channel_windows_of_wider_buffers(i, ins, outs):
    c, d = mr.PW_CASES[i], mr.pw_data(i, 'ints')
    xw = _wide(_dev(d['x'], ins), c.cin + 16, 8, POISON)
    out = torch.full(mr.pw_out_shape(c)[:-1] + (c.cout + 16,), SENT, dtype=_dt(outs), device=DEV)
    _pw(c, d, ins, outs, x=xw, out=out, in_ch_off=8, out_ch_off=8)
    _exactly(out[..., 8:8 + c.cout], d['y'], outs, _name(c, ins, outs) + ' windows')
    assert _untouched_outside(out, 8, c.cout)


# ---- pcp_mp_pointwise_wgrad ----------------------------------------------------------------------------------------------------------------

def _pwg(a, b, n, k, rows, out, **kw):
    tops = _mods()[2]
    return tops.pointwise_wgrad(tops.rowmap(a, n, **kw.pop('ka', {})), tops.rowmap(b, k, **kw.pop('kb', {})), rows, out, **kw)


@pytest.mark.parametrize('i', range(len(mr.PWG_CASES)))
def test_pointwise_wgrad_integer_inputs_bit_for_bit_then_accumulated(i):
    """the exact sums, then accumulate=1 onto an integer-filled out: old + sums, exactly"""
    c, d = mr.PWG_CASES[i], mr.pwg_data(i, True)
    a, b = _dev(d['a'], 'bf16'), _dev(d['b'], 'bf16')
    what = 'wgrad %dx%d rows %d' % (c.n, c.k, c.rows)
    got = torch.full((c.n, c.k), SENT, device=DEV)
    _pwg(a, b, c.n, c.k, c.rows, got)
    _exactly(got, d['out'], 'f32', what)
    old = mr.pwg_old(i)
    got = _dev(old)
    _pwg(a, b, c.n, c.k, c.rows, got, accumulate=True)
    _exactly(got, mr.f64(old) + d['out'], 'f32', what + ' accumulate')


@pytest.mark.parametrize('side', ['a', 'b'])
def test_pointwise_wgrad_lattice_row_maps_bit_for_bit(side):
    """all four taps of the lattice of WGRAD_LATTICE on one operand, the identity on the other; integers"""
    n, k = mr.WGRAD_LATTICE[:2]
    d = mr.lattice_data(side)
    rows = d['rows']
    bd, sd = _dev(d['big'], 'bf16'), _dev(d['small'], 'bf16')
    for tap, (lat, want, _S) in enumerate(d['taps']):
        got = torch.full((n, k), SENT, device=DEV)
        if side == 'a':
            _pwg(bd, sd, n, k, rows, got, ka=dict(lattice=lat))
        else:
            _pwg(sd, bd, n, k, rows, got, kb=dict(lattice=lat))
        _exactly(got, want, 'f32', 'wgrad lattice on %s, tap %d' % (side, tap))


@pytest.mark.parametrize('i', range(len(mr.PWG_CASES)))
def test_pointwise_wgrad_float_inputs_within_the_bound(i):
    c, d = mr.PWG_CASES[i], mr.pwg_data(i, False)
    got = torch.full((c.n, c.k), SENT, device=DEV)
    _pwg(_dev(d['a'], 'bf16'), _dev(d['b'], 'bf16'), c.n, c.k, c.rows, got)
    _within(got, dict(pre=d['out'], y=d['out'], S=d['S'], K=d['K'], relu=False), 'f32', 'wgrad %dx%d rows %d' % (c.n, c.k, c.rows))


# ---- e. determinism and refusals -----------------------------------------------------------------------------------------------------------

def test_second_launches_give_the_same_bits():
    """once per kernel, on float inputs where another summation order would show"""
    c, d = mr.FAST_CASES[6], mr.conv_data('fast', 6, 'float')
    assert c.th == 0 and _same_bits(_conv(c, d, 'bf16', 'f32'), _conv(c, d, 'bf16', 'f32'))
    c, d = mr.GEN_CASES[4], mr.conv_data('gen', 4, 'float')
    assert _same_bits(_conv(c, d, 'f32', 'f32'), _conv(c, d, 'f32', 'f32'))
    c, d = mr.PW_CASES[4], mr.pw_data(4, 'float')
    assert _same_bits(_pw(c, d, 'bf16', 'f32'), _pw(c, d, 'bf16', 'f32'))
    i = len(mr.PWG_CASES) - 2                                                # the largest: 258 stages over 32 splits
    c, d = mr.PWG_CASES[i], mr.pwg_data(i, False)
    a, b = _dev(d['a'], 'bf16'), _dev(d['b'], 'bf16')
    one, two = torch.full((c.n, c.k), SENT, device=DEV), torch.zeros((c.n, c.k), device=DEV)
    _pwg(a, b, c.n, c.k, c.rows, one)
    _pwg(a, b, c.n, c.k, c.rows, two)
    torch.cuda.synchronize()
    assert _same_bits(one, two)


def test_documented_refusals_return_their_code_and_leave_the_output_untouched():
    """every call here returns from the argument checks, before any launch"""
    lib, ops, _tops = _mods()
    L = lib.load()
    x = torch.ones((1, 4, 4, 64), dtype=torch.bfloat16, device=DEV)
    wp = torch.zeros(4 * 9 * 2 * 64 * 8, dtype=torch.bfloat16, device=DEV)   # never read
    bias = torch.zeros(128, device=DEV)
    out = torch.full((1, 4, 4, 64), SENT, device=DEV)

    def conv(in_off=0, **kw):
        f = dict(batch=1, in_h=4, in_w=4, cin=32, cout=64, cout_pad=64, stride=1, ld_in=64, ld_out=64, relu=0, in_dtype=lib.DT_BF16,
                 out_dtype=lib.DT_F32)
        f.update(kw)
        d = lib.MpConv3x3(**f)
        return L.pcp_mp_conv3x3(ctypes.byref(d), ctypes.c_void_p(x.data_ptr() + in_off), ops._p(wp), ops._p(bias), ops._p(out), ops._stream())
    assert conv(cin=24) == ARG                                               # cin % 16
    assert conv(cout_pad=96) == ARG                                          # cout_pad % 64
    assert conv(stride=3) == ARG and conv(stride=0) == ARG
    assert conv(in_dtype=2) == ARG and conv(out_dtype=-1) == ARG             # no such storage type
    assert conv(in_off=2) == ARG and conv(in_off=4) == ARG                   # bf16 input not 8-byte aligned
    assert conv(in_dtype=lib.DT_F32, ld_in=32, in_off=8) == ARG              # fp32 input not 16-byte aligned
    assert conv(ld_in=66) == ARG and conv(ld_out=66) == ARG                  # ld % 4

    def pw(in_off=0, **kw):
        f = dict(mode=lib.PW_PLAIN, rows=16, batch=1, in_h=4, in_w=4, cin=32, cout=64, cout_pad=64, ld_in=64, ld_out=64, relu=0,
                 in_dtype=lib.DT_BF16, out_dtype=lib.DT_F32)
        f.update(kw)
        d = lib.MpPointwise(**f)
        return L.pcp_mp_pointwise(ctypes.byref(d), ctypes.c_void_p(x.data_ptr() + in_off), ops._p(wp), ops._p(bias), ops._p(out), ops._stream())
    assert pw(cin=48) == UNSUPPORTED                                         # cin % 32: the caller keeps the fp32 entry point
    assert pw(cout=60) == UNSUPPORTED and pw(cout_pad=96) == UNSUPPORTED and pw(ld_in=68) == UNSUPPORTED
    assert pw(in_dtype=2) == ARG and pw(out_dtype=2) == ARG
    assert pw(mode=lib.PW_SPACE2DEPTH, in_h=3, in_w=4, cin=32, ld_in=64) == ARG    # odd in_h
    assert pw(mode=lib.PW_SPACE2DEPTH, in_h=4, in_w=3, cin=32, ld_in=64) == ARG
    assert pw(in_off=8) == ARG                                               # 16-byte aligned pointers
    torch.cuda.synchronize()
    assert _untouched_outside(out, 0, 0)
