"""The two 3x3 weight-gradient kernels, pcp_conv3x3_wgrad (fp32 MFMA, csrc/wgrad.hip) and pcp_mp_conv3x3_wgrad (bf16 MFMA,
csrc/mp_wgrad.hip), against the float64 reference and the case tables of tests/wgrad3x3_refs.py.  Integer inputs: bit-equality with the
float64 result.  Float inputs: the derived bound of tests/pointwise_refs.py element by element, (K + 2) * 2^-24 * S with K = B * Ho * Wo
and nothing on top for fp32, twice that on the bf16-rounded operands for bf16 (the matrix unit's adds may truncate).  Each bound comparison
prints the largest |got - ref| / bound it saw (pytest -s).  GPU only.

Measured on the MI355X, largest |got - ref| / bound per case of the tables, in table order (the bf16 ratios are against 2 * bound):
  fp32  0.27862 0.01375 0.00451 0.00046 0.00009 0.00443 | stride 2: 0.32802 0.00215 0.00468 0.00066
  bf16  0.03804 0.00496 0.00056 0.00032 0.00005 0.00053 0.00224 | stride 2: 0.00000 0.00033 0.00040 0.00119
  channel windows (2, 10, 34), 8 -> 8 and 72 -> 40 at strides 1, 2: fp32 0.00065 0.00356 0.00089 0.00546, bf16 0.00021 0.00099 0.00040 0.00195
The worst-case bound grows with K while rounding errors grow with its square root, hence the small ratios of the large maps; the two maps with a
single output pixel (K = 1) come within a third of it.  What the bound cannot see at the large maps, the integer variants do: on them
both kernels are exact (the bf16 matrix unit sums small integers exactly), and so is accumulate=True onto them.
"""
import ctypes

import numpy as np
import pytest
import torch

import wgrad3x3_refs as wr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.678                # what every float a launch must not write holds before it
NAN = float('nan')               # what every float a launch must not READ holds
ARG, WORKSPACE = 1, 2            # PCP_ERR_ARG, PCP_ERR_WORKSPACE of include/pcp_hip.h
KINDS = ('fp32', 'bf16')
CASES = [(k, i) for k in KINDS for i in range(len(wr.TABLES[k]))]


def _mods():
    from pcp_amd import lib, ops, train_ops
    return lib, ops, train_ops


def _dtype(kind):
    return torch.float32 if kind == 'fp32' else torch.bfloat16


def _dev(a, kind='fp32'):
    """float32 host array -> device tensor of the kernel's storage type (the bf16 tables hold values exact in bf16)"""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).to(_dtype(kind))


def _call(kind, x, dy, c, dw, **kw):
    tops = _mods()[2]
    f = tops.conv3x3_wgrad if kind == 'fp32' else tops.mp_conv3x3_wgrad
    return f(x, dy, c.cin, c.cout, c.stride, dw, **kw)


def _fresh_dw(c, fill=SENT):
    return torch.full((c.cout, c.cin, 3, 3), fill, dtype=torch.float32, device=DEV)


def _run_case(kind, i, ints, **kw):
    c, d = wr.TABLES[kind][i], wr.case_data(kind, i, ints)
    x, dy = _dev(d['x'], kind), _dev(d['dy'], kind)
    dw = _fresh_dw(c)
    _call(kind, x, dy, c, dw, **kw)
    return c, d, x, dy, dw


def _name(kind, c):
    return '%s (%d,%d,%d) %d->%d s%d' % (kind, c.B, c.H, c.W, c.cin, c.cout, c.stride)


def _exactly(got, want, what):
    """the float32 tensor holds the float64 array bit for bit (every value here is finite; 0 == -0)"""
    torch.cuda.synchronize()
    g = got.detach().cpu().double().numpy()
    assert g.shape == want.shape, (g.shape, want.shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    bad = g != want
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements differ, largest difference %g; first at [co, ci, ky, kx] = %s: got %r, want %r; taps hit '
                             '(ky, kx): %s' % (what, int(bad.sum()), bad.size, float(np.abs(g - want).max()), at, g[at], want[at],
                                               sorted({(int(a[2]), int(a[3])) for a in np.argwhere(bad)})))


def _within(got, ref, S, K, factor, what):
    """|got - ref| <= factor * bound(S, K) at every element; prints and returns the largest ratio"""
    torch.cuda.synchronize()
    g = got.detach().cpu().double().numpy()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    err, bnd = np.abs(g - ref), factor * wr.bound(S, K)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    print('\nRATIO %-44s max |got - ref| / (%d * bound) = %.5f' % (what, factor, worst))
    bad = int((err > bnd).sum())
    assert bad == 0, '%s: %d of %d elements outside the bound, worst ratio %.3f' % (what, bad, err.size, worst)
    return worst


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_sentinel(buf):
    sent = torch.tensor(SENT, dtype=torch.float32).view(torch.int32).item()
    return bool((buf.contiguous().view(torch.int32) == sent).all())


def _wide(inner, ld, off, fill):
    """`inner` (..., c) placed at channels [off, off + c) of a (..., ld) buffer of the same type that holds `fill` everywhere else"""
    buf = torch.full(tuple(inner.shape[:-1]) + (ld,), fill, dtype=inner.dtype, device=DEV)
    buf[..., off:off + inner.shape[-1]] = inner
    return buf


# ---- a. exact integers ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,i', CASES)
def test_integer_inputs_give_the_float64_result_bit_for_bit(kind, i):
    """every product and partial sum is an integer below 2^24 (asserted on the CPU): any summation order, split plan and storage type owes
    the exact result, and one dropped, doubled or misplaced pixel changes an integer; then accumulate=True onto it: exactly twice"""
    c, d, x, dy, dw = _run_case(kind, i, True)
    _exactly(dw, d['dw'], _name(kind, c))
    _call(kind, x, dy, c, dw, accumulate=True)
    _exactly(dw, 2 * d['dw'], _name(kind, c) + ' accumulate')


# ---- b. one-hot placement ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('kind', KINDS)
def test_one_hot_dy_copies_the_patch_of_x_bit_for_bit(kind, stride):
    """dy = 1.0 at one (b, oy, ox, co), 0 elsewhere: dw[co, :, ky, kx] is x[b, oy s + ky - 1, ox s + kx - 1, :] (a sum of one value and
    zeros), exactly 0 for the taps that leave the map, and every other co is exactly 0.  Pixels: the map corners, either side of a tile
    boundary (fp32) or of a strip and a row-split boundary (bf16) in each direction, an interior one"""
    c, x = wr.PLACE[(kind, stride)], wr.place_x(kind, stride)
    Ho, Wo = wr.out_hw(c.H, c.W, stride)
    xd = _dev(x, kind)
    for n, (what, b, oy, ox) in enumerate(wr.place_pixels(kind, stride)):
        co = (3 * n + 1) % c.cout
        dy = torch.zeros((c.B, Ho, Wo, c.cout), dtype=_dtype(kind), device=DEV)
        dy[b, oy, ox, co] = 1.0
        dw = _fresh_dw(c)
        _call(kind, xd, dy, c, dw)
        want = np.zeros((c.cout, c.cin, 3, 3), np.float64)
        want[co] = wr.one_hot_expect(x, b, oy, ox, stride)
        _exactly(dw, want, '%s one-hot at b %d (%d, %d), %s' % (_name(kind, c), b, oy, ox, what))


# ---- c. float inputs against the bound ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,i', CASES)
def test_float_inputs_within_the_bound(kind, i):
    c, d, _x, _dy, dw = _run_case(kind, i, False)
    _within(dw, d['dw'], d['S'], d['K'], 1 if kind == 'fp32' else 2, _name(kind, c))


# ---- d. channel windows with poison ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cin,cout', [(8, 8), (72, 40)])
@pytest.mark.parametrize('kind', KINDS)
def test_channel_windows_of_nan_filled_buffers(kind, cin, cout, stride):
    """x and dy are channel windows at non-zero offsets of wider buffers whose other channels are NaN: a read outside a window reaches dw.
    The kernel stages the same values in the same order as for the compact copies, so the two results have the same bits.  (The bf16
    kernel copies 128-byte records: with 8 or 72 channels a record reaches past the window, and for the last pixels it reached past the
    buffer until pcp_mp_conv3x3_wgrad ended its buffer ranges at the last window; such a read changes no result and cannot be asserted on)"""
    c = wr.Case(2, 10, 34, cin, cout, stride, 'ragged tiles and a second strip of two columns at stride 1, one ragged strip at stride 2')
    Ho, Wo = wr.out_hw(c.H, c.W, stride)
    x, dy = wr.make_inputs(kind, 3000 + cin + stride, (c.B, c.H, c.W, cin), (c.B, Ho, Wo, cout), False)
    ref, S = wr.wgrad3x3(x, dy, stride)
    xd, dyd = _dev(x, kind), _dev(dy, kind)
    compact = _fresh_dw(c)
    _call(kind, xd, dyd, c, compact)
    x_off, dy_off = (8, 4) if kind == 'fp32' else (16, 8)                     # 16-byte aligned windows
    xw, dyw = _wide(xd, cin + x_off + 12 - 4 * (kind == 'bf16'), x_off, NAN), _wide(dyd, cout + dy_off + 16, dy_off, NAN)
    assert bool(torch.isnan(xw[..., x_off - 1]).all()) and bool(torch.isnan(xw[..., x_off + cin]).all())
    assert bool(torch.isnan(dyw[..., dy_off - 1]).all()) and bool(torch.isnan(dyw[..., dy_off + cout]).all())
    dw = _fresh_dw(c)
    _call(kind, xw, dyw, c, dw, x_ch_off=x_off, dy_ch_off=dy_off)
    _within(dw, ref, S, c.B * Ho * Wo, 1 if kind == 'fp32' else 2, _name(kind, c) + ' windows')
    assert _same_bits(dw, compact)


# ---- e. workspace hygiene ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS)
def test_every_call_rewrites_the_partial_sums_it_reduces(kind):
    """the wrappers share one grow-only workspace.  The largest case leaves it large and dirty; it is then filled with NaN before each of
    the smallest cases and the 72 -> 40 one: a partial tile that is reduced but was not written by THIS call shows as a NaN, and
    otherwise as a result that differs from the exact one"""
    tops = _mods()[2]
    big = wr.largest(kind)
    c, d, _x, _dy, dw = _run_case(kind, big, True)
    _exactly(dw, d['dw'], _name(kind, c))
    ws = tops._WG_WS.buf
    assert ws is not None and ws.is_cuda and ws.numel() % 4 == 0 and ws.numel() > (8 << 20)
    small = [(B, H, W, ci, co, s) for B, H, W, ci, co, s, _why in wr.TABLES[kind]
             if (ci, co) == (72, 40) or (ci, co) == (8, 8)]
    assert len(small) == 3                                                   # the smallest map of either stride, and 72 -> 40
    for shape in small:
        ws.view(torch.float32).fill_(NAN)
        i = wr.index_of(kind, *shape)
        c, d, _x, _dy, dw = _run_case(kind, i, True)
        assert tops._WG_WS.buf is ws                                         # the buffer that was poisoned is the one the call used
        _exactly(dw, d['dw'], _name(kind, c) + ' on a NaN-filled workspace')
    assert bool(torch.isnan(ws.view(torch.float32)[-1]))                     # and the small calls left its far end alone


# ---- f. determinism and surroundings -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,shape', [('fp32', (4, 24, 48, 256, 256, 1)), ('fp32', (2, 18, 34, 64, 64, 2)),
                                        ('bf16', (1, 40, 64, 64, 64, 1)), ('bf16', (2, 18, 66, 64, 64, 2))])
def test_two_launches_give_the_same_bits(kind, shape):
    """both headers promise a fixed reduction order; split cases with float inputs, where another order would show"""
    i = wr.index_of(kind, *shape)
    c, _d, x, dy, first = _run_case(kind, i, False)
    again = _fresh_dw(c, 0.0)
    _call(kind, x, dy, c, again)
    torch.cuda.synchronize()
    assert _same_bits(again, first)


@pytest.mark.parametrize('kind', KINDS)
def test_nothing_around_dw_is_written(kind):
    i = wr.index_of(kind, 2, 16, 32, 72, 40, 1) if kind == 'fp32' else wr.index_of(kind, 2, 12, 31, 72, 40, 1)
    c, d = wr.TABLES[kind][i], wr.case_data(kind, i, True)
    n, guard = c.cout * c.cin * 9, 256
    buf = torch.full((guard + n + guard,), SENT, dtype=torch.float32, device=DEV)
    dw = buf[guard:guard + n].view(c.cout, c.cin, 3, 3)
    for acc in (False, True):
        _call(kind, _dev(d['x'], kind), _dev(d['dy'], kind), c, dw, accumulate=acc)
        _exactly(dw, (2 if acc else 1) * d['dw'], _name(kind, c) + ' inside a larger buffer')
        assert _all_sentinel(buf[:guard]) and _all_sentinel(buf[guard + n:])


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------------

def _refused(call, dw):
    lib = _mods()[0]
    with pytest.raises(lib.PcpError):
        call()
    torch.cuda.synchronize()
    assert _all_sentinel(dw)


def _maps(kind, B, H, W, ld_x, ld_dy, stride):
    return (torch.ones((B, H, W, ld_x), dtype=_dtype(kind), device=DEV),
            torch.ones((B, H // stride, W // stride, ld_dy), dtype=_dtype(kind), device=DEV))


@pytest.mark.parametrize('kind', KINDS)
def test_refusals_leave_dw_untouched(kind):
    m = 4 if kind == 'fp32' else 8                                           # the kernel's channel multiple
    for H, W in ((5, 6), (6, 5)):                                            # stride 2 on an odd map
        c = wr.Case(1, H, W, 8, 8, 2, '')
        x, dy = _maps(kind, 1, H, W, 8, 8, 2)
        dw = _fresh_dw(c)
        _refused(lambda: _call(kind, x, dy, c, dw), dw)
    x, dy = _maps(kind, 1, 4, 4, 16, 16, 1)
    for cin, cout in ((m - 2, m), (m, m - 2), (m + 2, m), (m, m + 2)):       # channels outside the multiple, inside 16-wide buffers
        c = wr.Case(1, 4, 4, cin, cout, 1, '')
        dw = _fresh_dw(c)
        _refused(lambda: _call(kind, x, dy, c, dw), dw)
    c = wr.Case(1, 4, 4, m, m, 1, '')
    dw = _fresh_dw(c)
    for kw in (dict(x_ch_off=m // 4), dict(dy_ch_off=m // 2), dict(x_ch_off=m - 1)):      # windows that start 4 / 8 / 12 or 14 bytes into a 16-byte unit
        _refused(lambda: _call(kind, x, dy, c, dw, **kw), dw)
    _call(kind, x, dy, c, dw, x_ch_off=m, dy_ch_off=m)                       # and an aligned window of the same buffers is accepted
    _exactly(dw, wr.wgrad3x3(np.ones((1, 4, 4, m), np.float32), np.ones((1, 4, 4, m), np.float32), 1)[0], 'ones')


def test_bf16_entry_refuses_channel_counts_the_wrapper_hands_to_the_fp32_kernel():
    """cin or cout a multiple of 4 but not of 8: mp_conv3x3_wgrad runs the fp32 kernel on fp32 copies (its documented route for shapes
    the bf16 kernel has no plan for), so the refusal of the bf16 entry itself is checked through the C call"""
    lib, ops, tops = _mods()
    L = lib.load()
    x, dy = _maps('bf16', 1, 4, 4, 16, 16, 1)
    dw = torch.full((16, 16, 3, 3), SENT, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for cin, cout in ((12, 8), (8, 12), (0, 8), (8, 0), (24, 8), (8, 24)):    # the last two: more channels than the 16-wide pixel records hold
        d = lib.MpWgrad3x3(1, 4, 4, cin, cout, 1, 16, 16, lib.DT_BF16, lib.DT_BF16, 0)
        assert L.pcp_mp_conv3x3_wgrad_workspace_bytes(ctypes.byref(d)) == 0
        _refused(lambda: lib.check(L.pcp_mp_conv3x3_wgrad(ctypes.byref(d), ops._p(x), ops._p(dy), ops._p(dw), ops._p(ws), ws.numel(), ops._stream()),
                                   'pcp_mp_conv3x3_wgrad'), dw)
    c = wr.Case(1, 4, 4, 12, 8, 1, '')
    got = _fresh_dw(c)
    tops.mp_conv3x3_wgrad(x, dy, 12, 8, 1, got)                              # the wrapper's route: the same sums, from the fp32 kernel
    _exactly(got, wr.wgrad3x3(np.ones((1, 4, 4, 12), np.float32), np.ones((1, 4, 4, 8), np.float32), 1)[0], 'bf16 wrapper, cin 12')


@pytest.mark.parametrize('kind', KINDS)
def test_workspace_one_byte_short_is_refused(kind):
    lib, ops, _tops = _mods()
    L = lib.load()
    i = wr.index_of(kind, 2, 16, 32, 72, 40, 1) if kind == 'fp32' else wr.index_of(kind, 2, 12, 31, 72, 40, 1)
    c, d = wr.TABLES[kind][i], wr.case_data(kind, i, True)
    x, dy = _dev(d['x'], kind), _dev(d['dy'], kind)
    dw = _fresh_dw(c)
    if kind == 'fp32':
        desc = lib.Conv3x3(c.B, c.H, c.W, c.cin, c.cout, 0, c.stride, c.cin, c.cout, 0)
        need = L.pcp_conv3x3_wgrad_workspace_bytes(ctypes.byref(desc))
        _ty, _tx, _n, nsplit = wr.plan_fp32(*c[:6])
        assert need == nsplit * 9 * 128 * 64 * 4                             # [nsplit][9][cout_r][cin_r] floats
    else:
        desc = lib.MpWgrad3x3(c.B, c.H, c.W, c.cin, c.cout, c.stride, c.cin, c.cout, lib.DT_BF16, lib.DT_BF16, 0)
        need = L.pcp_mp_conv3x3_wgrad_workspace_bytes(ctypes.byref(desc))
        assert need == 2 * wr.plan_bf16(*c[:6])[3] * 9 * 64 * 64 * 4         # [pair][split] tiles of 9 x 64 x 64 floats
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(ws_bytes):
        if kind == 'fp32':
            return L.pcp_conv3x3_wgrad(ctypes.byref(desc), ops._p(x), ops._p(dy), ops._p(ws), ws_bytes, ops._p(dw), 0, ops._stream())
        return L.pcp_mp_conv3x3_wgrad(ctypes.byref(desc), ops._p(x), ops._p(dy), ops._p(dw), ops._p(ws), ws_bytes, ops._stream())
    assert call(need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert _all_sentinel(dw)
    assert call(need) == 0                                                   # and the same arguments, whole, are accepted
    _exactly(dw, d['dw'], _name(kind, c) + ' on a workspace of exactly the size asked for')
