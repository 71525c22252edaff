"""The float64 references and case tables of tests/pointwise_refs.py, checked on the CPU: the references against torch's own float64
convolutions and autograd, the tables against the properties they claim (computed from pack.py and the kernels' documented constants, not
from the kernels), and the tolerance against three deliberate faults it has to be able to see.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_refs as pr
from pcp_amd import pack

PLAIN_IDS = range(len(pr.PLAIN_CASES))
S2D_IDS = range(len(pr.S2D_CASES))
D2S_IDS = range(len(pr.D2S_CASES))
SPATIAL = [('s2d', i) for i in S2D_IDS] + [('d2s', i) for i in D2S_IDS]


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _close(got, want):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float(np.abs(got - want).max()) <= 1e-12, float(np.abs(got - want).max())


# ---- the references against torch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', PLAIN_IDS)
def test_plain_reference_equals_conv2d_in_float64(i):
    c, d = pr.PLAIN_CASES[i], pr.plain_data(i)
    y = F.conv2d(_t(d['x']).t().reshape(1, c.cin, c.rows, 1), _t(d['w'])[:, :, None, None], _t(d['b']))[0, :, :, 0].t()
    if c.res == 'before':
        y = F.relu(y + _t(d['res']))
    else:
        y = F.relu(y) if c.relu else y
        y = y + _t(d['res']) if c.res else y
    _close(d['y'], y)
    # S from the definition, one row at a time
    r = c.rows // 2
    S = (np.abs(pr.f64(d['x'][r]))[None, :] * np.abs(pr.f64(d['w']))).sum(1) + np.abs(pr.f64(d['b']))
    if c.res:
        S = S + np.abs(pr.f64(d['res'][r]))
    assert np.allclose(d['S'][r], S, rtol=1e-13, atol=0)
    assert d['K'] == c.cin and (d['S'] > 0).all()


@pytest.mark.parametrize('kind,i', SPATIAL)
def test_spatial_references_equal_torch_convs_in_float64(kind, i):
    c, d = (pr.S2D_CASES if kind == 's2d' else pr.D2S_CASES)[i], pr.spatial_data(kind, i)
    if kind == 's2d':
        y = F.conv2d(_nchw(d['x']), _t(d['w']), _t(d['b']), stride=2)
    else:
        y = F.conv_transpose2d(_nchw(d['x']), _t(d['w']), _t(d['b']), stride=2)
    y = F.relu(y) if c.relu else y
    _close(d['y'], y.permute(0, 2, 3, 1))
    # S is the same operation on the absolute values (+ |b|)
    if kind == 's2d':
        S = F.conv2d(_nchw(d['x']).abs(), _t(d['w']).abs(), _t(d['b']).abs(), stride=2)
    else:
        S = F.conv_transpose2d(_nchw(d['x']).abs(), _t(d['w']).abs(), _t(d['b']).abs(), stride=2)
    assert np.allclose(d['S'], S.permute(0, 2, 3, 1).numpy(), rtol=1e-13, atol=0)
    assert d['K'] == (4 * c.cin if kind == 's2d' else c.cin)


def _layer(kind, cin, cout):
    if kind == 'plain':
        return torch.nn.Conv2d(cin, cout, 1, bias=True).double()
    if kind == 's2d':
        return torch.nn.Conv2d(cin, cout, 2, stride=2, bias=True).double()
    return torch.nn.ConvTranspose2d(cin, cout, 2, stride=2, bias=True).double()


@pytest.mark.parametrize('kind', ['plain', 's2d', 'd2s'])
def test_pw_wgrad_reference_equals_autograd_weight_gradient(kind):
    """the assembly the layers use: plain = one product; Conv2d k2 s2 = one product per tap with the lattice on the INPUT side;
    ConvTranspose2d k2 s2 = one per tap with the lattice on the OUTPUT-gradient side"""
    n, k, B, gh, gw = pr.WGRAD_LATTICE
    cin, cout = k, n
    H, W = (gh, gw) if kind != 's2d' else (2 * gh, 2 * gw)
    layer = _layer(kind, cin, cout)
    x = pr.uniform(501, 1, (B, H, W, cin))
    y = layer(_nchw(x))
    dy = pr.uniform(501, 2, tuple(y.permute(0, 2, 3, 1).shape))
    (y * _nchw(dy)).sum().backward()
    want = layer.weight.grad.numpy()
    rows = B * gh * gw
    if kind == 'plain':
        got, S = pr.pw_wgrad(dy, x, None, None, rows)
        _close(got.reshape(cout, cin, 1, 1), want)
        assert S.shape == (cout, cin) and (S >= np.abs(got)).all()
    elif kind == 's2d':
        taps = [pr.pw_wgrad(dy, x, None, (gh, gw, t // 2, t % 2), rows)[0] for t in range(4)]
        _close(np.stack(taps, -1).reshape(cout, cin, 2, 2), want)
    else:
        taps = [pr.pw_wgrad(x, dy, None, (gh, gw, t // 2, t % 2), rows)[0] for t in range(4)]
        _close(np.stack(taps, -1).reshape(cin, cout, 2, 2), want)


def test_map_rows_is_the_lattice_of_the_header():
    gh, gw = 2, 3
    for ky in (0, 1):
        for kx in (0, 1):
            m = pr.map_rows(2 * gh * gw, (gh, gw, ky, kx))
            want = [(b * 2 * gh + 2 * y + ky) * 2 * gw + 2 * x + kx for b in range(2) for y in range(gh) for x in range(gw)]
            assert m.tolist() == want
    assert pr.map_rows(5, None).tolist() == [0, 1, 2, 3, 4]


def test_selection_references_are_gathers():
    """with 0/1 selection weights and zero bias the references return the selected inputs exactly"""
    c = pr.PLACE_PLAIN
    w, pick = pr.selection_plain(1, c.cout, c.cin)
    x = pr.small_ints(601, 1, (c.rows, c.cin))
    y, _ = pr.plain(x, w, np.zeros(c.cout, np.float32))
    assert np.array_equal(y, pr.f64(x)[:, pick]) and (x != 0).all() and np.abs(x).max() <= 16 and np.array_equal(x, np.round(x))


# ---- the tables hold what they claim ---------------------------------------------------------------------------------------------------

def _cout_pad(kind, cout):
    """from pack.py, on zero weights"""
    z = torch.zeros
    if kind == 'plain':
        return pack.pack_plain(z(cout, 16), z(cout))[2]
    if kind == 's2d':
        return pack.pack_conv2x2_s2(z(cout, 16, 2, 2), z(cout))[2]
    return pack.pack_convT2x2_s2(z(16, cout, 2, 2), z(cout))[2]


def _rows(kind, c):
    return c.rows if kind == 'plain' else (c.B * (c.H // 2) * (c.W // 2) if kind == 's2d' else c.B * c.H * c.W)


TABLES = {'plain': pr.PLAIN_CASES, 's2d': pr.S2D_CASES, 'd2s': pr.D2S_CASES}


@pytest.mark.parametrize('kind', ['plain', 's2d', 'd2s'])
def test_forward_tables_cover_both_instantiations_and_ragged_rows(kind):
    cases = TABLES[kind]
    pads = {_cout_pad(kind, c.cout) for c in cases}
    assert all(_cout_pad(kind, c.cout) == pr.cout_pad_of(c.cout) for c in cases)
    assert any(p % 64 == 32 for p in pads) and any(p % 64 == 0 for p in pads)              # 128x32 and 128x64
    assert any(_rows(kind, c) % pr.BM != 0 for c in cases) and any(_rows(kind, c) > pr.BM for c in cases)
    assert {True, False} <= {c.relu for c in cases}
    if kind == 'plain':
        assert {1, 127, 128, 129} <= {c.rows for c in cases}
    else:
        assert any(c.H != c.W for c in cases) and {1, 3} <= {c.B for c in cases}
        if kind == 's2d':
            assert all(c.H % 2 == 0 and c.W % 2 == 0 for c in cases)


def test_forward_tables_cover_the_channel_counts():
    for kind, cases in TABLES.items():
        cins = {c.cin for c in cases}
        assert {16, 48, 256} <= cins, (kind, cins)                                         # one slice, odd slice count, many
        assert all(c.cin % pr.CK == 0 for c in cases)
    assert {1, 9, 20, 32, 70, 128} <= {c.cout for c in pr.PLAIN_CASES}
    for kind in ('s2d', 'd2s'):
        assert {1, 9, 20, 32, 70, 128} <= {c.cout for c in TABLES[kind]}
    with_res = [c for c in pr.PLAIN_CASES if c.res]
    for tail in (1, 2, 3):
        assert {'after', 'before'} <= {c.res for c in with_res if c.cout % 4 == tail}, tail
    assert all(c.relu for c in with_res if c.res == 'before')
    splits = [c for c in pr.PLAIN_CASES if c.k_split]
    assert {c.k_split for c in splits if c.cin == 64} >= {16, 64 - 16, 64 // 2}
    assert all(0 < c.k_split < c.cin and c.k_split % pr.CK == 0 and c.rows % pr.BM != 0 for c in splits)


def test_residual_orders_differ_at_most_elements():
    for i, c in enumerate(pr.PLAIN_CASES):
        if not c.res or not c.relu:
            continue
        d = pr.plain_data(i)
        acc, S = pr.plain_acc(d['x'][:, :c.k_split] if c.k_split else d['x'], d['w'], d['x'][:, c.k_split:] if c.k_split else None, c.k_split)
        after, _ = pr.finish(acc, S, d['b'], d['res'], True, False)
        before, _ = pr.finish(acc, S, d['b'], d['res'], True, True)
        differ = np.abs(after - before) > pr.bound(d['S'], d['K'])
        assert differ.mean() > 0.5, (i, differ.mean())


def test_wgrad_table_runs_the_chunk_loop_more_than_once():
    shapes = {(c.n, c.k) for c in pr.WGRAD_CASES}
    assert {(4, 4), (72, 40), (64, 64), (128, 260), (256, 256)} <= shapes
    assert {1, 127, 128, 129} <= {c.rows for c in pr.WGRAD_CASES if (c.n, c.k) == (64, 64)}
    assert all(c.n % 4 == 0 and c.k % 4 == 0 for c in pr.WGRAD_CASES)
    # the rule, restated here: 128 rows per chunk, nsplit = min(512 / pairs, 256, chunks)
    plans = []
    for c in pr.WGRAD_CASES:
        chunks = -(-c.rows // 128)
        pairs = -(-c.n // 64) * -(-c.k // 64)
        nsplit = min(512 // pairs, 256, chunks)
        assert (chunks, nsplit) == pr.pw_split(c.rows, c.n, c.k)
        plans.append((c, chunks, nsplit))
    multi = [(c, ch, ns) for c, ch, ns in plans if ch > ns and ch % ns != 0]
    assert multi and any((c.n, c.k, c.rows, ch, ns) == (256, 256, 8229, 65, 32) for c, ch, ns in multi)
    assert any(ch == ns and ch > 1 for _c, ch, ns in plans)                                # and the one-trip form the layer tests see


# ---- the tolerance can see a real fault ------------------------------------------------------------------------------------------------

FACTOR = 100.0


def _seen(faulty, d):
    """the fault moves at least one element by more than FACTOR times that element's bound"""
    return bool((np.abs(faulty - d['y']) > FACTOR * pr.bound(d['S'], d['K'])).any())


def _plain_parts(c, d):
    if c.k_split:
        return d['x'][:, :c.k_split], d['x'][:, c.k_split:]
    return d['x'], None


@pytest.mark.parametrize('i', PLAIN_IDS)
def test_bound_sees_a_dropped_slice_and_a_misplaced_residual_plain(i):
    c, d = pr.PLAIN_CASES[i], pr.plain_data(i)
    x1, x2 = _plain_parts(c, d)
    for s in {0, c.cin // pr.CK - 1, (c.cin // pr.CK) // 2}:
        w = d['w'].copy()
        w[:, s * pr.CK:(s + 1) * pr.CK] = 0
        acc, S = pr.plain_acc(x1, w, x2, c.k_split)
        y, _ = pr.finish(acc, S, d['b'], d['res'], c.relu, c.res == 'before')
        assert _seen(y, d), ('dropped slice', s)
    if c.res and c.relu:
        acc, S = pr.plain_acc(x1, d['w'], x2, c.k_split)
        y, _ = pr.finish(acc, S, d['b'], d['res'], True, c.res != 'before')
        assert _seen(y, d), 'residual on the wrong side of the ReLU'


@pytest.mark.parametrize('kind,i', SPATIAL)
def test_bound_sees_a_dropped_slice_and_a_shifted_tap_spatial(kind, i):
    c, d = (pr.S2D_CASES if kind == 's2d' else pr.D2S_CASES)[i], pr.spatial_data(kind, i)
    ref = pr.space2depth if kind == 's2d' else pr.depth2space
    n_sl = c.cin // pr.CK
    for tap, s in ((0, 0), (3, n_sl - 1), (2, n_sl // 2)):
        w = d['w'].copy()
        if kind == 's2d':
            w[:, s * pr.CK:(s + 1) * pr.CK, tap >> 1, tap & 1] = 0                         # one K slice = 16 channels of one tap
        else:
            w[s * pr.CK:(s + 1) * pr.CK] = 0                                               # one K slice = 16 input channels, all taps
        assert _seen(ref(d['x'], w, d['b'], c.relu)[0], d), ('dropped slice', tap, s)
    for tap in range(4):
        ky, kx = tap >> 1, tap & 1
        if kind == 's2d':
            # the tap reads the pixel next to its own: (2y + ky, 2x + 1 - kx)
            taps = pr.space2depth_taps(d['x'], d['w'])
            wt = pr.f64(d['w'])[:, :, ky, kx]
            taps[tap] = (pr.f64(pr.tap_pixels(d['x'], ky, 1 - kx)) @ wt.T, taps[tap][1])
            y, _ = pr.finish(sum(t[0] for t in taps), 0.0, d['b'], relu=c.relu)
        else:
            # the tap's plane lands one pixel aside, on its row neighbour's pixels (and that one's here)
            planes = [t[0] for t in pr.depth2space_taps(d['x'], d['w'])]
            other = ky * 2 + (1 - kx)
            planes[tap], planes[other] = planes[other], planes[tap]
            y, _ = pr.finish(pr.interleave_taps(planes), 0.0, d['b'], relu=c.relu)
        assert _seen(y, d), ('shifted tap', tap)


@pytest.mark.parametrize('i', range(len(pr.WGRAD_CASES)))
def test_bound_sees_a_lost_chunk_wgrad(i):
    """the weight gradient's bound grows with rows * S, so at 8229 rows it is about 1 against entries of about 30: still, ONE lost chunk of
    128 rows (of 65) moves most entries past it -- a chunk fetched twice, skipped or overwritten in LDS cannot hide inside the tolerance"""
    c, d = pr.WGRAD_CASES[i], pr.wgrad_data(i)
    lost = pr.pw_wgrad(d['a'][:128], d['b'][:128], None, None, min(128, c.rows))[0]
    assert (np.abs(lost) > pr.bound(d['S'], d['K'])).mean() > 0.5
