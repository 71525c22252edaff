"""pcp_pointwise (fp32: 1x1 / Linear, Conv2d k2 s2, ConvTranspose2d k2 s2) and pcp_pointwise_wgrad on fp32 operands against the float64
references of tests/pointwise_refs.py.  Every tolerance is the derived bound of that file, (K + 2) * 2^-24 * S element by element with
nothing on top, or bit-equality.  Each comparison prints the largest |got - ref| / bound it saw (pytest -s).  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_refs as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.678                # what every float a launch must not write holds before it
NAN = float('nan')               # what every float a launch must not READ holds


def _mods():
    from pcp_amd import lib, ops, pack, train_ops
    return lib, ops, pack, train_ops


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def _pack(kind, w, b):
    _lib, _ops, pack, _t = _mods()
    w, b = torch.from_numpy(np.array(w)), torch.from_numpy(np.array(b))
    f = {'plain': pack.pack_plain, 's2d': pack.pack_conv2x2_s2, 'd2s': pack.pack_convT2x2_s2}[kind]
    wp, bp, cp = f(w, b)
    return wp.to(DEV), bp.to(DEV), cp


def _mode(kind):
    lib = _mods()[0]
    return {'plain': lib.PW_PLAIN, 's2d': lib.PW_SPACE2DEPTH, 'd2s': lib.PW_DEPTH2SPACE}[kind]


def _within(got, y, S, K, what):
    """|got - ref| <= bound(S, K) at every element; prints the largest ratio"""
    torch.cuda.synchronize()
    g = got.detach().cpu().numpy().astype(np.float64)
    assert g.shape == y.shape, (g.shape, y.shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    err, bnd = np.abs(g - y), pr.bound(S, K)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    print('\nRATIO %-72s max |got - ref| / bound = %.5f' % (what, float(ratio.max())))
    bad = int((err > bnd).sum())
    assert bad == 0, '%s: %d of %d elements outside the bound, worst ratio %.3f' % (what, bad, err.size, float(ratio.max()))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _wide(inner, ld, off, fill):
    """`inner` (..., c) placed at channels [off, off + c) of a (..., ld) buffer that holds `fill` everywhere else"""
    inner = inner if isinstance(inner, torch.Tensor) else _dev(inner)
    buf = torch.full(tuple(inner.shape[:-1]) + (ld,), fill, dtype=torch.float32, device=DEV)
    buf[..., off:off + inner.shape[-1]] = inner
    return buf


def _untouched_outside(buf, off, c):
    """every float of `buf` outside channels [off, off + c) still holds the bits of SENT"""
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[off:off + c] = False
    sent = torch.tensor(SENT, dtype=torch.float32).view(torch.int32).item()
    return bool((buf.view(torch.int32)[..., keep] == sent).all())


def _all_sentinel(buf):
    return _untouched_outside(buf, 0, 0)


# ---- forward, all three modes, over the tables ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', range(len(pr.PLAIN_CASES)))
def test_plain_forward_within_the_bound(i):
    lib, ops, _p, _t = _mods()
    c, d = pr.PLAIN_CASES[i], pr.plain_data(i)
    wp, bp, cp = _pack('plain', d['w'], d['b'])
    assert cp == pr.cout_pad_of(c.cout)
    kw = {}
    x = _dev(d['x'])
    if c.k_split:
        x, kw['x2'], kw['k_split'] = _dev(d['x'][:, :c.k_split]), _dev(d['x'][:, c.k_split:]), c.k_split
    if c.res:
        kw['residual'], kw['residual_before_relu'] = _dev(d['res']), c.res == 'before'
    got = ops.pointwise(x, wp, bp, lib.PW_PLAIN, c.cin, c.cout, cp, relu=c.relu, **kw)
    _within(got, d['y'], d['S'], d['K'], 'plain[%d] %dx%d->%d' % (i, c.rows, c.cin, c.cout))


@pytest.mark.parametrize('kind,i', [('s2d', i) for i in range(len(pr.S2D_CASES))] + [('d2s', i) for i in range(len(pr.D2S_CASES))])
def test_spatial_forward_within_the_bound(kind, i):
    _lib, ops, _p, _t = _mods()
    c, d = (pr.S2D_CASES if kind == 's2d' else pr.D2S_CASES)[i], pr.spatial_data(kind, i)
    wp, bp, cp = _pack(kind, d['w'], d['b'])
    assert cp == pr.cout_pad_of(c.cout)
    got = ops.pointwise(_dev(d['x']), wp, bp, _mode(kind), c.cin, c.cout, cp, relu=c.relu)
    _within(got, d['y'], d['S'], d['K'], '%s[%d] (%d,%d,%d) %d->%d' % (kind, i, c.B, c.H, c.W, c.cin, c.cout))


# ---- exact placement ---------------------------------------------------------------------------------------------------------------------

def test_plain_selection_weights_copy_the_selected_channels_bit_for_bit():
    lib, ops, _p, _t = _mods()
    c = pr.PLACE_PLAIN
    w, pick = pr.selection_plain(1, c.cout, c.cin)
    x = pr.small_ints(601, 1, (c.rows, c.cin))
    wp, bp, cp = _pack('plain', w, np.zeros(c.cout, np.float32))
    got = ops.pointwise(_dev(x), wp, bp, lib.PW_PLAIN, c.cin, c.cout, cp, relu=False)
    assert _same_bits(got, _dev(x[:, pick]))


def test_space2depth_selection_weights_copy_one_tap_and_channel_bit_for_bit():
    lib, ops, _p, _t = _mods()
    c = pr.PLACE_S2D
    sel, pick = pr.selection_plain(2, c.cout, 4 * c.cin)                  # pick = tap * cin + channel
    assert len({int(p) // c.cin for p in pick}) == 4                        # every tap is somebody's source
    w = np.zeros((c.cout, c.cin, 2, 2), np.float32)
    for n, p in enumerate(pick):
        w[n, p % c.cin, (p // c.cin) >> 1, (p // c.cin) & 1] = 1.0
    x = pr.small_ints(602, 1, (c.B, c.H, c.W, c.cin))
    want = np.stack([pr.tap_pixels(x, (p // c.cin) >> 1, (p // c.cin) & 1)[..., p % c.cin] for p in pick], -1)
    assert np.array_equal(pr.space2depth(x, w, np.zeros(c.cout))[0], want)
    wp, bp, cp = _pack('s2d', w, np.zeros(c.cout, np.float32))
    got = ops.pointwise(_dev(x), wp, bp, lib.PW_SPACE2DEPTH, c.cin, c.cout, cp, relu=False)
    assert _same_bits(got, _dev(want))


def test_depth2space_selection_weights_copy_per_tap_permutations_bit_for_bit():
    lib, ops, _p, _t = _mods()
    c = pr.PLACE_D2S
    w = np.zeros((c.cin, c.cout, 2, 2), np.float32)
    picks = []
    for tap in range(4):
        sel, pick = pr.selection_plain(10 + tap, c.cout, c.cin)
        w[:, :, tap >> 1, tap & 1] = sel.T
        picks.append(pick)
    assert len({tuple(p) for p in picks}) == 4                              # the taps differ: a plane in another tap's place shows
    x = pr.small_ints(603, 1, (c.B, c.H, c.W, c.cin))
    want = pr.interleave_taps([pr.f64(x)[..., p] for p in picks])
    assert np.array_equal(pr.depth2space(x, w, np.zeros(c.cout))[0], want)
    wp, bp, cp = _pack('d2s', w, np.zeros(c.cout, np.float32))
    got = ops.pointwise(_dev(x), wp, bp, lib.PW_DEPTH2SPACE, c.cin, c.cout, cp, relu=False)
    assert _same_bits(got, _dev(want))


# ---- channel windows ---------------------------------------------------------------------------------------------------------------------

# (ld_out, out_ch_off): 16-byte stores | scalar stores because of the offset | scalar stores because of the odd pixel stride
OUT_LAYOUTS = [(96, 8), (96, 6), (97, 8)]


@pytest.mark.parametrize('cout', [21, 70])
def test_plain_channel_windows_of_wider_buffers(cout):
    """x, x2, the residual and the output are windows at non-zero offsets of buffers of four different widths; what lies outside the input
    windows is NaN (a read there reaches the output), what lies outside the output window is a sentinel (a write there shows)"""
    lib, ops, _p, _t = _mods()
    rows, cin, ks = 150, 48, 32
    x = pr.uniform(701, 1, (rows, cin))
    w = pr.uniform(701, 2, (cout, cin), -0.1, 0.1)
    b = pr.uniform(701, 3, (cout,), -0.2, 0.2)
    res = pr.uniform(701, 4, (rows, cout))
    y, S = pr.plain(x, w, b, residual=res, relu=True)
    wp, bp, cp = _pack('plain', w, b)
    xw, x2w, rw = _wide(x[:, :ks], 44, 8, NAN), _wide(x[:, ks:], 28, 4, NAN), _wide(res, 83, 5, NAN)
    outs = []
    for ld_out, off in OUT_LAYOUTS:
        out = torch.full((rows, ld_out), SENT, device=DEV)
        ops.pointwise(xw, wp, bp, lib.PW_PLAIN, cin, cout, cp, relu=True, out=out, in_ch_off=8, out_ch_off=off, x2=x2w, k_split=ks,
                      x2_ch_off=4, residual=rw, res_ch_off=5)
        _within(out[:, off:off + cout], y, S, cin, 'plain window cout %d ld_out %d off %d' % (cout, ld_out, off))
        assert _untouched_outside(out, off, cout)
        outs.append(out[:, off:off + cout])
    assert _same_bits(outs[1], outs[0]) and _same_bits(outs[2], outs[0])    # the scalar epilogue stores what the 16-byte one does


@pytest.mark.parametrize('kind', ['s2d', 'd2s'])
def test_spatial_channel_windows_of_wider_buffers(kind):
    """the same for the two spatial modes; for depth-to-space the sentinel check spans the pixels of all four taps"""
    _lib, ops, _p, _t = _mods()
    B, H, W, cin, cout = (3, 6, 10, 32, 21) if kind == 's2d' else (3, 5, 7, 32, 21)
    x = pr.uniform(702, 1, (B, H, W, cin))
    w = pr.uniform(702, 2, (cout, cin, 2, 2) if kind == 's2d' else (cin, cout, 2, 2), -0.1, 0.1)
    b = pr.uniform(702, 3, (cout,), -0.2, 0.2)
    y, S = (pr.space2depth if kind == 's2d' else pr.depth2space)(x, w, b, False)
    K = 4 * cin if kind == 's2d' else cin
    wp, bp, cp = _pack(kind, w, b)
    xw = _wide(x, 44, 8, NAN)
    outs = []
    for ld_out, off in OUT_LAYOUTS:
        out = torch.full(tuple(y.shape[:3]) + (ld_out,), SENT, device=DEV)
        ops.pointwise(xw, wp, bp, _mode(kind), cin, cout, cp, relu=False, out=out, in_ch_off=8, out_ch_off=off)
        _within(out[..., off:off + cout], y, S, K, '%s window ld_out %d off %d' % (kind, ld_out, off))
        assert _untouched_outside(out, off, cout)
        outs.append(out[..., off:off + cout])
    assert _same_bits(outs[1], outs[0]) and _same_bits(outs[2], outs[0])


# ---- two-source K ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k_split', [16, 48, 32])
def test_two_source_k_equals_the_single_source_call_on_the_cat(k_split):
    """x2 supplies channels [k_split, cin) from a window of a wider buffer.  The kernel stages the same values in the same slice order as
    for the materialised cat, so beyond the bound the two results have the same bits: any difference is an addressing fault"""
    lib, ops, _p, _t = _mods()
    rows, cin, cout = 203, 64, 70
    x = pr.uniform(710 + k_split, 1, (rows, cin))
    w = pr.uniform(710 + k_split, 2, (cout, cin), -0.1, 0.1)
    b = pr.uniform(710 + k_split, 3, (cout,), -0.2, 0.2)
    y, S = pr.plain(x[:, :k_split], w, b, x[:, k_split:], k_split, relu=True)
    assert float(np.abs(y - pr.plain(x, w, b, relu=True)[0]).max()) <= 1e-12           # the reference of the cat, in another summation order
    wp, bp, cp = _pack('plain', w, b)
    x2w = _wide(x[:, k_split:], cin - k_split + 24, 12, NAN)
    got = ops.pointwise(_dev(x[:, :k_split]), wp, bp, lib.PW_PLAIN, cin, cout, cp, relu=True, x2=x2w, k_split=k_split, x2_ch_off=12)
    _within(got, y, S, cin, 'two-source k_split %d' % k_split)
    one = ops.pointwise(_dev(x), wp, bp, lib.PW_PLAIN, cin, cout, cp, relu=True)
    assert _same_bits(got, one)


# ---- residual ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cout', [9, 70, 11])
@pytest.mark.parametrize('before', [False, True])
def test_residual_after_and_inside_the_activation(cout, before):
    """cout % 4 = 1, 2, 3: the masked residual reads of the last channel quad.  The residual is a window of a wider buffer whose other floats,
    the one just past the last channel among them, are NaN; none may reach the output.  (The two orders differ at most elements, see
    test_residual_orders_differ_at_most_elements: a launch that took the other one cannot stay inside the bound.)"""
    lib, ops, _p, _t = _mods()
    rows, cin = 150, 48
    x = pr.uniform(720 + cout, 1, (rows, cin))
    w = pr.uniform(720 + cout, 2, (cout, cin), -0.1, 0.1)
    b = pr.uniform(720 + cout, 3, (cout,), -0.2, 0.2)
    res = pr.uniform(720 + cout, 4, (rows, cout))
    y, S = pr.plain(x, w, b, residual=res, relu=True, residual_before_relu=before)
    other = pr.plain(x, w, b, residual=res, relu=True, residual_before_relu=not before)[0]
    assert (np.abs(other - y) > pr.bound(S, cin)).mean() > 0.5
    wp, bp, cp = _pack('plain', w, b)
    rw = _wide(res, cout + 7, 3, NAN)
    assert bool(torch.isnan(rw[:, 3 + cout]).all())
    got = ops.pointwise(_dev(x), wp, bp, lib.PW_PLAIN, cin, cout, cp, relu=True, residual=rw, res_ch_off=3, residual_before_relu=before)
    _within(got, y, S, cin, 'residual %s cout %d' % ('inside' if before else 'after', cout))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def _refused(call, out):
    lib = _mods()[0]
    with pytest.raises(lib.PcpError):
        call()
    torch.cuda.synchronize()
    assert _all_sentinel(out)


def test_pointwise_refusals_leave_the_output_untouched():
    lib, ops, _p, _t = _mods()
    wp = torch.zeros(4 * 64 * 16, device=DEV)                               # never read: every call is refused before a launch
    bp = torch.zeros(64, device=DEV)
    out = torch.full((12, 32), SENT, device=DEV)
    x = torch.ones((12, 64), device=DEV)
    x2 = torch.ones((12, 64), device=DEV)
    P = lib.PW_PLAIN
    _refused(lambda: ops.pointwise(torch.ones((12, 24), device=DEV), wp, bp, P, 24, 32, 32, out=out), out)          # cin % 16
    for ks in (0, 64, 24):                                                                                           # k_split
        _refused(lambda: ops.pointwise(x, wp, bp, P, 64, 32, 32, out=out, x2=x2, k_split=ks), out)
    _refused(lambda: ops.pointwise(x, wp, bp, P, 32, 32, 32, out=out, in_ch_off=2), out)                             # 8-byte aligned input
    for H, W in ((5, 6), (6, 5)):                                                                                    # odd map, Conv2d k2 s2
        o4 = out.view(1, 2, 3, 64)
        _refused(lambda: ops.pointwise(torch.ones((1, H, W, 16), device=DEV), wp, bp, lib.PW_SPACE2DEPTH, 16, 32, 32, out=o4), out)
    # relu(. + residual) without a residual: through the C entry, the wrapper asserts before it
    d = lib.Pointwise(P, 12, 0, 0, 0, 64, 32, 32, 64, 32, lib.RELU_PRE_RESIDUAL)
    L = lib.load()
    _refused(lambda: lib.check(L.pcp_pointwise(ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(bp), ops._p(out), ops._stream()), 'pcp_pointwise'),
             out)


def test_pointwise_of_zero_rows_is_a_no_op():
    lib, ops, _p, _t = _mods()
    wp, bp = torch.zeros(64 * 16, device=DEV), torch.zeros(32, device=DEV)
    out = torch.full((4, 32), SENT, device=DEV)
    x = torch.ones((4, 16), device=DEV)
    # the C entry, at a valid address
    d = lib.Pointwise(lib.PW_PLAIN, 0, 0, 0, 0, 16, 32, 32, 16, 32, 1)
    assert lib.load().pcp_pointwise(ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(bp), ops._p(out), ops._stream()) == 0
    # the wrapper, on a zero-row tensor (torch gives it a null address, which the C entry would refuse)
    assert x[:0].shape == (0, 16)
    assert ops.pointwise(x[:0], wp, bp, lib.PW_PLAIN, 16, 32, 32, out=out) is out
    assert ops.pointwise(x[:0], wp, bp, lib.PW_PLAIN, 16, 32, 32).shape == (0, 32)
    torch.cuda.synchronize()
    assert _all_sentinel(out)


# ---- pcp_pointwise_wgrad on fp32 operands ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', range(len(pr.WGRAD_CASES)))
def test_wgrad_within_the_bound_and_repeatable(i):
    _lib, _ops, _p, tops = _mods()
    c, d = pr.WGRAD_CASES[i], pr.wgrad_data(i)
    a, b = _dev(d['a']), _dev(d['b'])
    got = torch.full((c.n, c.k), SENT, device=DEV)
    tops.pointwise_wgrad(tops.rowmap(a, c.n), tops.rowmap(b, c.k), c.rows, got)
    _within(got, d['out'], d['S'], d['K'], 'wgrad[%d] %dx%d rows %d' % (i, c.n, c.k, c.rows))
    again = torch.full((c.n, c.k), SENT, device=DEV)
    tops.pointwise_wgrad(tops.rowmap(a, c.n), tops.rowmap(b, c.k), c.rows, again)
    torch.cuda.synchronize()
    assert _same_bits(again, got)                                           # the header promises a fixed reduction order


@pytest.mark.parametrize('side', ['a', 'b'])
def test_wgrad_lattice_row_maps_on_a_non_square_grid(side):
    """all four taps, the lattice on one operand and the identity on the other, batch 3 on a 5 x 7 grid (rows run across map rows and
    across batch entries)"""
    _lib, _ops, _p, tops = _mods()
    n, k, B, gh, gw = pr.WGRAD_LATTICE
    rows = B * gh * gw
    big_c, small_c = (n, k) if side == 'a' else (k, n)
    big = pr.uniform(730, 1, (B, 2 * gh, 2 * gw, big_c))
    small = pr.uniform(730, 2, (rows, small_c))
    bd, sd = _dev(big), _dev(small)
    for tap in range(4):
        lat = (gh, gw, tap >> 1, tap & 1)
        got = torch.full((n, k), SENT, device=DEV)
        if side == 'a':
            want, S = pr.pw_wgrad(big, small, lat, None, rows)
            tops.pointwise_wgrad(tops.rowmap(bd, n, lattice=lat), tops.rowmap(sd, k), rows, got)
        else:
            want, S = pr.pw_wgrad(small, big, None, lat, rows)
            tops.pointwise_wgrad(tops.rowmap(sd, n), tops.rowmap(bd, k, lattice=lat), rows, got)
        _within(got, want, S, rows, 'wgrad lattice on %s, tap %d' % (side, tap))


def test_wgrad_operand_and_output_windows_and_accumulation():
    """operands as channel windows of wider buffers (NaN around them), out as a window of a wider matrix (ld_out > k, sentinels around
    it), then accumulate=True onto the non-zero contents: within the bound of old + grad"""
    _lib, _ops, _p, tops = _mods()
    n, k, rows = 72, 40, 300
    a = pr.uniform(740, 1, (rows, n))
    b = pr.uniform(740, 2, (rows, k))
    want, S = pr.pw_wgrad(a, b, None, None, rows)
    aw, bw = _wide(a, n + 12, 8, NAN), _wide(b, k + 20, 4, NAN)
    ra, rb = tops.rowmap(aw, n, ch_off=8), tops.rowmap(bw, k, ch_off=4)
    wide = torch.full((n + 3, k + 9), SENT, device=DEV)
    out = wide[2:2 + n, 5:5 + k]
    tops.pointwise_wgrad(ra, rb, rows, out)
    _within(out, want, S, rows, 'wgrad windows, ld_out %d > k %d' % (wide.shape[1], k))

    def frame_intact():
        keep = torch.ones_like(wide, dtype=torch.bool)
        keep[2:2 + n, 5:5 + k] = False
        sent = torch.tensor(SENT, dtype=torch.float32).view(torch.int32).item()
        return bool((wide.view(torch.int32)[keep] == sent).all())
    assert frame_intact()
    old = pr.uniform(740, 3, (n, k), -50.0, 50.0)
    out.copy_(_dev(old))
    tops.pointwise_wgrad(ra, rb, rows, out, accumulate=True)
    _within(out, pr.f64(old) + want, S + np.abs(pr.f64(old)), rows, 'wgrad accumulate onto non-zero contents')
    assert frame_intact()


def test_wgrad_refusals():
    lib, ops, _p, tops = _mods()
    L = lib.load()
    n, k, rows = 64, 64, 300
    a, b = torch.ones((rows, n + 8), device=DEV), torch.ones((rows, k + 8), device=DEV)
    out = torch.full((n, k), SENT, device=DEV)
    need = L.pcp_pointwise_wgrad_workspace_bytes(rows, n, k)
    chunks, nsplit = pr.pw_split(rows, n, k)
    assert need == nsplit * 64 * 64 * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(ra, rb, r, ws_bytes=need):
        return L.pcp_pointwise_wgrad(ctypes.byref(ra), ctypes.byref(rb), r, ops._p(ws), ws_bytes, ops._p(out), k, 0, ops._stream())
    ARG, WORKSPACE = 1, 2                                                   # PCP_ERR_ARG, PCP_ERR_WORKSPACE of include/pcp_hip.h
    assert call(tops.rowmap(a, n), tops.rowmap(b, k), rows, need - 1) == WORKSPACE
    assert call(tops.rowmap(a, 6), tops.rowmap(b, k), rows) == ARG                         # channels % 4
    assert call(tops.rowmap(a, n), tops.rowmap(b, 6), rows) == ARG
    assert call(tops.rowmap(a, n, ch_off=1), tops.rowmap(b, k), rows) == ARG               # operand base not 16-byte aligned
    assert call(tops.rowmap(a, n), tops.rowmap(b, k, ch_off=2), rows) == ARG
    assert call(tops.rowmap(a, n), tops.rowmap(b, k), 0) == ARG                            # rows <= 0
    assert call(tops.rowmap(a, n), tops.rowmap(b, k), -1) == ARG
    torch.cuda.synchronize()
    assert _all_sentinel(out)
    assert call(tops.rowmap(a, n), tops.rowmap(b, k), rows) == 0                           # and the same arguments, whole, are accepted
    torch.cuda.synchronize()
    assert bool((out == float(rows)).all())
