"""The train-mode BatchNorm kernels (statistics, normalise, backward, column sums, the split entry points of cross-rank BatchNorm) and the
optimiser kernels (gradient norm, fused clip + AdamW step) against the float64 references of tests/train_step_refs.py.  Every tolerance is
a derived bound of that file, element by element with nothing on top.  Each comparison prints 'RATIO <group> <what> <largest |got - ref| /
bound>' (pytest -s); the groups are stats, normalise, backward, split, colsum, norm, adam.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import train_step_refs as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.678                # what every float a launch must not write holds before it (rounded to the buffer's type)
HUGE = 1e30                      # what every float a launch must not READ holds
OK, ARG = 0, 1                   # PCP_OK, PCP_ERR_ARG of include/pcp_hip.h
STAT_KEYS = ('scale', 'shift', 'mean', 'invstd')


def _mods():
    from pcp_amd import lib, train_ops
    return lib, train_ops


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).to(dtype)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().float().cpu().numpy()


def _sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def _is_sent(t):
    return bool((t == torch.tensor(SENT, dtype=t.dtype, device=t.device)).all())


def _dt(flag):
    return torch.bfloat16 if flag else torch.float32


def _within(group, what, got, ref, bnd):
    g = _host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert g.shape == np.shape(ref), (what, g.shape, np.shape(ref))
    r = tr.worst(g, ref, bnd)
    print('\nRATIO %-9s %-64s %.5f' % (group, what, r))
    assert r <= 1.0, '%s: |got - ref| / bound = %r' % (what, r)


def _vec(c, arrays):
    _lib, tops = _mods()
    v = tops.BNVectors(c, DEV)
    for name, a in zip(STAT_KEYS, arrays):
        getattr(v, name).copy_(_dev(a))
    return v


def _check_stats(group, what, vec, rm, rv, st):
    for k in STAT_KEYS:
        _within(group, '%s %s' % (what, k), getattr(vec, k), st[k], st['b_' + k])
    if rm is not None:
        _within(group, what + ' running_mean', rm, st['running_mean'], st['b_running_mean'])
        _within(group, what + ' running_var', rv, st['running_var'], st['b_running_var'])


def _check_backward(group, what, dg, db, dx, ref):
    _within(group, what + ' dgamma', dg, ref['dgamma'], ref['b_dgamma'])
    _within(group, what + ' dbeta', db, ref['dbeta'], ref['b_dbeta'])
    _within(group, what + ' dx', dx, ref['dx'], ref['b_dx'])


# ---- BatchNorm: statistics, normalise, backward over the shape table and the offset cases ----------------------------------------------------

@pytest.mark.parametrize('relu', (0, 1))
@pytest.mark.parametrize('i', range(len(tr.BN_CASES)))
def test_bn_stats_normalise_backward_within_the_bounds(i, relu):
    """three independent checks: the statistics against the reference, the normalisation on the KERNEL's vectors, the backward pass on
    the REFERENCE's vectors (rounded to float32)"""
    _lib, tops = _mods()
    case, d = tr.BN_CASES[i], tr.bn_data(i)
    c, what = case.c, '(%d, %d) %s eps=%g relu=%d' % (case.rows, case.c, case.kind, case.eps, relu)
    x = _dev(d['x'])
    rm, rv = _dev(d['rm']), _dev(d['rv'])
    vec = tops.bn_train_stats(x, c, _dev(d['gamma']), _dev(d['beta']), case.eps, tr.MOMENTUM, rm, rv)
    _check_stats('stats', what, vec, rm, rv, d['stats'])
    out = _sent(tuple(x.shape))
    tops.scale_shift_act(x, c, vec, bool(relu), out)
    y, b = tr.scale_shift_act(d['x'], _host(vec.scale), _host(vec.shift), relu)
    _within('normalise', what, out, y, b)
    if relu:
        assert float(out.min()) >= 0.0
    dout = _dev(d['dout'])
    dg, db, dx = _sent((c,)), _sent((c,)), _sent(tuple(x.shape))
    tops.bn_act_backward(dout, x, c, _vec(c, d['vec']), bool(relu), dg, db, dx=dx)
    _check_backward('backward', what, dg, db, dx, tr.bn_backward_data(i, bool(relu)))
    assert torch.equal(dout, _dev(d['dout'])) and torch.equal(x, _dev(d['x']))


def test_bn_planted_ties_get_no_gradient():
    """x scale + shift == 0 exactly at a tenth of the elements, dout == 1 there: act > 0 is false, so they add nothing to dgamma / dbeta
    and their dx holds the two mean terms only"""
    _lib, tops = _mods()
    t, c = tr.ties_data(), tr.BN_TIES.c
    dg, db, dx = _sent((c,)), _sent((c,)), _sent(t['x'].shape)
    tops.bn_act_backward(_dev(t['dout']), _dev(t['x']), c, _vec(c, t['vec']), True, dg, db, dx=dx)
    _check_backward('backward', 'planted ties', dg, db, dx, t['ref'])


@pytest.mark.parametrize('i', tr.BN_WINDOW)
def test_bn_channel_windows(i):
    """ld = c + 16, ch_off = 8 on x, dout, dx and out: 1e30 outside the window of every input, a sentinel outside it in every output"""
    _lib, tops = _mods()
    case, d = tr.BN_CASES[i], tr.bn_data(i)
    c, ld, off, what = case.c, case.c + 16, 8, 'window (%d, %d)' % (case.rows, case.c)

    def wide(a, fill):
        buf = torch.full((case.rows, ld), fill, dtype=torch.float32, device=DEV)
        if a is not None:
            buf[:, off:off + c] = _dev(a)
        return buf

    def outside_is_sent(buf):
        return _is_sent(buf[:, :off]) and _is_sent(buf[:, off + c:])

    x, dout = wide(d['x'], HUGE), wide(d['dout'], HUGE)
    rm, rv = _dev(d['rm']), _dev(d['rv'])
    vec = tops.bn_train_stats(x, c, _dev(d['gamma']), _dev(d['beta']), case.eps, tr.MOMENTUM, rm, rv, ch_off=off)
    _check_stats('stats', what, vec, rm, rv, d['stats'])
    out = wide(None, SENT)
    tops.scale_shift_act(x, c, vec, True, out, in_ch_off=off, out_ch_off=off)
    y, b = tr.scale_shift_act(d['x'], _host(vec.scale), _host(vec.shift), True)
    _within('normalise', what, out[:, off:off + c], y, b)
    assert outside_is_sent(out)
    dg, db, dx = _sent((c,)), _sent((c,)), wide(None, SENT)
    tops.bn_act_backward(dout, x, c, _vec(c, d['vec']), True, dg, db, dx=dx, dout_ch_off=off, x_ch_off=off, dx_ch_off=off)
    _check_backward('backward', what, dg, db, dx[:, off:off + c], tr.bn_backward_data(i, True))
    assert outside_is_sent(dx)
    cs = _sent((c,))
    tops.colsum(x, c, cs, ch_off=off)
    _within('colsum', what, cs, *tr.colsum(d['x']))


def test_bn_backward_accumulates_and_runs_in_place():
    _lib, tops = _mods()
    i = 5
    case, d, ref = tr.BN_CASES[i], tr.bn_data(i), tr.bn_backward_data(i, True)
    c = case.c
    x, vec = _dev(d['x']), _vec(c, d['vec'])
    g0, b0 = tr.uniform(800, 1, (c,), -3.0, 3.0), tr.uniform(800, 2, (c,), -3.0, 3.0)
    dg, db = _dev(g0), _dev(b0)
    for _ in range(2):
        dog = _dev(d['dout'])
        assert tops.bn_act_backward(dog, x, c, vec, True, dg, db, accumulate=True) is dog          # dx is dout
        _within('backward', 'in place dx', dog, ref['dx'], ref['b_dx'])
    _within('backward', 'accumulate twice dgamma', dg, tr.f64(g0) + 2 * ref['dgamma'],
            tr.accum_bound([g0, ref['dgamma'], ref['dgamma']], [ref['b_dgamma']] * 2))
    _within('backward', 'accumulate twice dbeta', db, tr.f64(b0) + 2 * ref['dbeta'],
            tr.accum_bound([b0, ref['dbeta'], ref['dbeta']], [ref['b_dbeta']] * 2))


@pytest.mark.parametrize('bx,bd,bo', [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
def test_bn_storage_types(bx, bd, bo):
    """x, dout, dx each float32 or bf16 at (3000, 64); the normalised output takes dx's type.  dgamma is checked: the reference's mask is
    the kernel's"""
    _lib, tops = _mods()
    case, d = tr.BN_STORAGE, tr.storage_data(bool(bx), bool(bd))
    c, what = case.c, 'storage x=%s dout=%s dx=%s' % tuple('bf16' if f else 'f32' for f in (bx, bd, bo))
    x = _dev(d['x'], _dt(bx))
    rm, rv = _dev(d['rm']), _dev(d['rv'])
    vec = tops.bn_train_stats(x, c, _dev(d['gamma']), _dev(d['beta']), case.eps, tr.MOMENTUM, rm, rv)
    _check_stats('stats', what, vec, rm, rv, d['stats'])
    out = _sent(tuple(x.shape), _dt(bo))
    tops.scale_shift_act(x, c, vec, True, out)
    _within('normalise', what, out, *tr.scale_shift_act(d['x'], _host(vec.scale), _host(vec.shift), True, bf16_out=bool(bo)))
    dg, db, dx = _sent((c,)), _sent((c,)), _sent(tuple(x.shape), _dt(bo))
    tops.bn_act_backward(_dev(d['dout'], _dt(bd)), x, c, _vec(c, d['vec']), True, dg, db, dx=dx)
    _check_backward('backward', what, dg, db, dx, tr.bn_backward(d['dout'], d['x'], *d['vec'], True, bf16_dx=bool(bo)))


def test_bn_refusals_return_err_arg_and_launch_nothing():
    lib, tops = _mods()
    L, p, cp, st = lib.load(), tops._p, tops._chan_ptr, tops._stream()
    F, B = lib.DT_F32, lib.DT_BF16
    big = torch.ones((8, 1056), device=DEV)                       # every (rows, ld) below fits in it
    ones = torch.ones((4, 1056), device=DEV)
    outs = _sent((8, 1056))
    vo, rm, rv, dg, db = _sent((4, 1056)), _sent((1056,)), _sent((1056,)), _sent((1056,)), _sent((1056,))
    sums = torch.full((2 * 1056,), SENT, dtype=torch.float64, device=DEV)
    ws = torch.empty(L.pcp_bn_workspace_bytes(1056), dtype=torch.uint8, device=DEV)

    def stats(xp, rows, c, ld, rmean=rm, rvar=rv):
        return L.pcp_bn_train_stats(xp, rows, c, ld, p(ones[0]), p(ones[1]), 1e-3, 0.01, p(rmean), p(rvar), p(ws), p(vo[0]), p(vo[1]), p(vo[2]),
                                    p(vo[3]), st)

    def backward(dp, ld_d, xp, ld_x, rows, c, dxp, ld_dx):
        return L.pcp_bn_act_backward(dp, ld_d, xp, ld_x, rows, c, p(ones[0]), p(ones[1]), p(ones[2]), p(ones[3]), 1, p(ws), p(dg), p(db), 0, dxp,
                                     ld_dx, st)

    shapes = {'c = 6': (8, 6, 8), 'c = 1028': (8, 1028, 1028), 'ld % 4 != 0': (8, 64, 66), 'ld < c': (8, 64, 32), 'rows = 0': (0, 64, 64)}
    for why, (rows, c, ld) in shapes.items():
        assert stats(p(big), rows, c, ld) == ARG, why
        assert backward(p(big), 64 if ld == 66 else ld, p(big), ld, rows, c, p(outs), 64 if ld == 66 else ld) == ARG, why
        assert L.pcp_bn_train_sums(p(big), rows, c, ld, p(ws), p(sums), st) == ARG, why
        assert L.pcp_bn_bwd_sums(p(big), 64, p(big), ld, rows, c, p(ones[0]), p(ones[1]), p(ones[2]), p(ones[3]), 1, p(ws), p(sums), st) == ARG, why
        assert L.pcp_colsum(p(big), rows, c, ld, p(ws), p(dg), 0, st) == ARG, why
        if why != 'c = 1028' and why != 'ld < c':                 # the element-wise kernel has no channel cap and no ld >= c rule of its own
            assert L.pcp_scale_shift_act(p(big), rows, c, ld, p(ones[0]), p(ones[1]), 1, p(outs), ld, st) == ARG, why
    assert backward(p(big), 66, p(big), 64, 8, 64, p(outs), 64) == ARG and backward(p(big), 64, p(big), 64, 8, 64, p(outs), 66) == ARG
    # a float32 window has to start at a multiple of four channels
    assert stats(cp(big, 2), 8, 64, 128) == ARG
    assert backward(cp(big, 2), 128, p(big), 128, 8, 64, p(outs), 128) == ARG
    assert backward(p(big), 128, cp(big, 2), 128, 8, 64, p(outs), 128) == ARG
    assert backward(p(big), 128, p(big), 128, 8, 64, cp(outs, 2), 128) == ARG
    assert L.pcp_scale_shift_act(cp(big, 2), 8, 64, 128, p(ones[0]), p(ones[1]), 1, p(outs), 128, st) == ARG
    assert L.pcp_scale_shift_act(p(big), 8, 64, 128, p(ones[0]), p(ones[1]), 1, cp(outs, 2), 128, st) == ARG
    # one running statistic without the other
    assert stats(p(big), 8, 64, 64, rmean=None) == ARG and stats(p(big), 8, 64, 64, rvar=None) == ARG
    assert L.pcp_bn_train_stats_from_sums(p(sums), 8, 64, p(ones[0]), p(ones[1]), 1e-3, 0.01, p(rm), None, p(vo[0]), p(vo[1]), p(vo[2]), p(vo[3]),
                                          st) == ARG
    # in place only at one storage type
    assert L.pcp_mp_bn_act_backward(p(outs), F, 64, p(big), F, 64, 8, 64, p(ones[0]), p(ones[1]), p(ones[2]), p(ones[3]), 1, p(ws), p(dg), p(db),
                                    0, p(outs), B, 64, st) == ARG
    torch.cuda.synchronize()
    for t in (outs, vo, rm, rv, dg, db):
        assert _is_sent(t)
    assert bool((sums == SENT).all())
    # and the same calls are taken once the argument is right
    assert stats(p(big), 8, 64, 64) == OK and backward(p(big), 64, p(big), 64, 8, 64, p(outs), 64) == OK
    torch.cuda.synchronize()
    assert not _is_sent(vo[:, :64]) and _is_sent(vo[:, 64:])


# ---- the split (cross-rank) entry points, called as the wrappers call them, the all-reduce replaced by a sum on the device ------------------

@pytest.mark.parametrize('form', ('f32', 'mp_f32', 'mp_bf16'))
@pytest.mark.parametrize('split', tr.SPLITS)
def test_bn_split_entry_points_meet_the_reference_on_the_union(split, form):
    lib, tops = _mods()
    L, p, st = lib.load(), tops._p, tops._stream()
    bf = form == 'mp_bf16'
    case, d = tr.BN_SPLIT, tr.split_data(bf)
    rows, c = case.rows, case.c
    assert sum(split) == rows
    dt, code = _dt(bf), (lib.DT_BF16 if bf else lib.DT_F32)
    x, dout = _dev(d['x'], dt), _dev(d['dout'])
    ws = tops._BN_WS.get(L.pcp_bn_workspace_bytes(c), x.device)
    shards = [(0, split[0]), (split[0], rows)]
    what = 'split %s %s' % (split, form)

    def rowp(t, a):
        return ctypes.c_void_p(t.data_ptr() + a * c * t.element_size())

    def nan64():
        return torch.full((2 * c,), float('nan'), dtype=torch.float64, device=DEV)

    # forward: sums per shard, added in float64, statistics from the sum on every shard
    parts = []
    for a, b in shards:
        s = nan64()
        if form == 'f32':
            assert L.pcp_bn_train_sums(rowp(x, a), b - a, c, c, p(ws), p(s), st) == OK
        else:
            assert L.pcp_mp_bn_train_sums(rowp(x, a), code, b - a, c, c, p(ws), p(s), st) == OK
        parts.append(s)
    tot = parts[0] + parts[1]
    x64 = tr.f64(d['x'])
    torch.cuda.synchronize()
    got = tot.cpu().numpy()
    assert tr.worst(got[:c], x64.sum(0), rows * tr.U64 * np.abs(x64).sum(0)) <= 1.0
    assert tr.worst(got[c:], (x64 * x64).sum(0), rows * tr.U64 * (x64 * x64).sum(0)) <= 1.0
    for a, b in shards:
        vec, rm, rv = tops.BNVectors(c, DEV), _dev(d['rm']), _dev(d['rv'])
        assert L.pcp_bn_train_stats_from_sums(p(tot), rows, c, p(_dev(d['gamma'])), p(_dev(d['beta'])), case.eps, tr.MOMENTUM, p(rm), p(rv),
                                              p(vec.scale), p(vec.shift), p(vec.mean), p(vec.invstd), st) == OK
        _check_stats('split', '%s rows [%d, %d)' % (what, a, b), vec, rm, rv, d['stats'])

    # backward: the two gradient sums per shard, dx from the sums over the union, dgamma / dbeta from the shard's own
    vr = _vec(c, d['vec'])
    vp = (p(vr.scale), p(vr.shift), p(vr.mean), p(vr.invstd))
    local = []
    for a, b in shards:
        s = nan64()
        if form == 'f32':
            assert L.pcp_bn_bwd_sums(rowp(dout, a), c, rowp(x, a), c, b - a, c, *vp, 1, p(ws), p(s), st) == OK
        else:
            assert L.pcp_mp_bn_bwd_sums(rowp(dout, a), lib.DT_F32, c, rowp(x, a), code, c, b - a, c, *vp, 1, p(ws), p(s), st) == OK
        local.append(s)
    glob = local[0] + local[1]
    union = tr.bn_backward(d['dout'], d['x'], *d['vec'], True, bf16_dx=bf)
    for (a, b), loc in zip(shards, local):
        dg, db, dx = _sent((c,)), _sent((c,)), _sent((b - a, c), dt)
        if form == 'f32':
            rc = L.pcp_bn_bwd_apply_from_sums(rowp(dout, a), c, rowp(x, a), c, b - a, c, *vp, 1, p(loc), p(glob), rows, p(ws), p(dg), p(db), 0, p(dx),
                                              c, st)
        else:
            rc = L.pcp_mp_bn_bwd_apply_from_sums(rowp(dout, a), lib.DT_F32, c, rowp(x, a), code, c, b - a, c, *vp, 1, p(loc), p(glob), rows, p(ws),
                                                 p(dg), p(db), 0, p(dx), code, c, st)
        assert rc == OK
        shard = tr.bn_backward(d['dout'][a:b], d['x'][a:b], *d['vec'], True)
        w = '%s rows [%d, %d)' % (what, a, b)
        _within('split', w + ' dgamma', dg, shard['dgamma'], shard['b_dgamma'])
        _within('split', w + ' dbeta', db, shard['dbeta'], shard['b_dbeta'])
        _within('split', w + ' dx', dx, union['dx'][a:b], union['b_dx'][a:b])
    # fewer rows in total than on this shard: refused, nothing written
    a, b = shards[1]
    dg, db, dx = _sent((c,)), _sent((c,)), _sent((b - a, c))
    if form == 'f32':
        assert L.pcp_bn_bwd_apply_from_sums(rowp(dout, a), c, rowp(x, a), c, b - a, c, *vp, 1, p(local[1]), p(glob), b - a - 1, p(ws), p(dg), p(db), 0,
                                            p(dx), c, st) == ARG
        torch.cuda.synchronize()
        assert _is_sent(dg) and _is_sent(db) and _is_sent(dx)


def test_bn_stats_from_sums_takes_six_channels():
    """the finalize step has no four-channel layout: c = 6 is legal there"""
    lib, tops = _mods()
    L, p, st = lib.load(), tops._p, tops._stream()
    rows, c = 100, 6
    x = tr.uniform(810, 1, (rows, c), -2.0, 3.0)
    gamma, beta, rm, rv = (tr.uniform(810, k, (c,), lo, hi) for k, lo, hi in ((2, 0.5, 1.5), (3, -0.2, 0.2), (4, -0.1, 0.1), (5, 0.5, 1.5)))
    ref = tr.bn_stats(x, gamma, beta, 1e-3, tr.MOMENTUM, rm, rv)
    x64 = tr.f64(x)
    sums = torch.from_numpy(np.concatenate([x64.sum(0), (x64 * x64).sum(0)])).to(DEV)
    vec, rmd, rvd = _sent((4, 8)), _dev(rm), _dev(rv)
    assert L.pcp_bn_train_stats_from_sums(p(sums), rows, c, p(_dev(gamma)), p(_dev(beta)), 1e-3, tr.MOMENTUM, p(rmd), p(rvd), p(vec[0]), p(vec[1]),
                                          p(vec[2]), p(vec[3]), st) == OK
    for k, name in enumerate(STAT_KEYS):
        _within('split', 'stats_from_sums c=6 ' + name, vec[k, :c], ref[name], ref['b_' + name])
    _within('split', 'stats_from_sums c=6 running_mean', rmd, ref['running_mean'], ref['b_running_mean'])
    _within('split', 'stats_from_sums c=6 running_var', rvd, ref['running_var'], ref['b_running_var'])
    assert _is_sent(vec[:, c:])


# ---- colsum ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', tr.COLSUM_CASES)
def test_colsum_within_the_bound(i):
    _lib, tops = _mods()
    case, d = tr.BN_CASES[i], tr.bn_data(i)
    s, b = tr.colsum(d['x'])
    out = _sent((case.c,))
    tops.colsum(_dev(d['x']), case.c, out)
    _within('colsum', '(%d, %d)' % (case.rows, case.c), out, s, b)


def test_colsum_bf16_input_and_accumulate():
    _lib, tops = _mods()
    d, c = tr.storage_data(True, False), tr.BN_STORAGE.c
    s, b = tr.colsum(d['x'])
    init = tr.uniform(820, 1, (c,), -50.0, 50.0)
    out = _dev(init)
    x = _dev(d['x'], torch.bfloat16)
    tops.colsum(x, c, out, accumulate=True)
    tops.colsum(x, c, out, accumulate=True)
    _within('colsum', 'bf16 input, accumulated twice', out, tr.f64(init) + 2 * s, tr.accum_bound([init, s, s], [b, b]))
    tops.colsum(x, c, out)
    _within('colsum', 'bf16 input', out, s, b)


# ---- gradient norm -----------------------------------------------------------------------------------------------------------------------------

def _sqnorm_of(g, acc=None, accumulate=False):
    """pcp_grad_sqnorm on the first g.size floats of a larger 16-byte aligned buffer (a pointer even for n = 0) -> the device scalar"""
    lib, tops = _mods()
    buf = torch.zeros(g.size + 4, device=DEV)
    buf[:g.size] = _dev(g)
    if acc is None:
        acc = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)           # accumulate = 0 has to overwrite it
    assert buf.data_ptr() % 16 == 0
    assert lib.load().pcp_grad_sqnorm(tops._p(buf), g.size, tops._p(acc), 1 if accumulate else 0, tops._stream()) == OK
    return acc


def _norm_within(what, acc, ref, bnd):
    torch.cuda.synchronize()
    got = float(acc.item())
    r = abs(got - ref) / bnd if bnd > 0 else (0.0 if got == ref else float('inf'))
    print('\nRATIO %-9s %-64s %.5f' % ('norm', what, r))
    assert r <= 1.0, (what, got, ref, bnd)


@pytest.mark.parametrize('n', tr.NORM_NS)
def test_sqnorm_within_the_bound(n):
    g = tr.norm_grad(n)
    _norm_within('n = %d' % n, _sqnorm_of(g), *tr.sqnorm(g))


def test_sqnorm_accumulates_over_two_buffers():
    a, b = tr.norm_grad(1023), tr.norm_grad(5)
    acc = _sqnorm_of(a)
    _sqnorm_of(b, acc, accumulate=True)
    _norm_within('1023 + 5 accumulated', acc, *tr.sqnorm(np.concatenate([a, b])))
    before = float(acc.item())
    _sqnorm_of(tr.norm_grad(0), acc, accumulate=True)
    torch.cuda.synchronize()
    assert float(acc.item()) == before


@pytest.mark.parametrize('huge', (1e19, 3e19))
def test_sqnorm_keeps_an_element_whose_square_leaves_float32(huge):
    """1e19^2 = 1e38 is at the top of float32 (any second such element overflows the sum), (3e19)^2 is past it: the squares are float64"""
    g = np.array(tr.norm_grad(1023))
    g[500] = huge
    s, b = tr.sqnorm(g)
    assert s > 0.99 * float(np.float32(huge)) ** 2
    _norm_within('one element of %g' % huge, _sqnorm_of(g), s, b)


def test_sqnorm_refuses_a_pointer_off_16_bytes():
    lib, tops = _mods()
    buf = torch.ones(64, device=DEV)
    acc = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)
    assert lib.load().pcp_grad_sqnorm(tops._chan_ptr(buf, 1), 8, tops._p(acc), 0, tops._stream()) == ARG
    torch.cuda.synchronize()
    assert float(acc.item()) == 123.0


# ---- Adam step ---------------------------------------------------------------------------------------------------------------------------------

def _gpu_adam(case):
    """(step_fn, sqnorm_fn) for train_step_refs.adam_run: the norm kernel's own result is what the step is handed AND what the reference reads"""
    _lib, tops = _mods()
    held = {}

    def sqnorm_fn(g):
        held['g'] = _dev(g)
        held['sq'] = tops.grad_sqnorm(held['g'])
        torch.cuda.synchronize()
        return float(held['sq'].item())

    def place(a, off):
        buf = _sent((a.size + 8,))
        buf[off:off + a.size] = _dev(a)
        return buf, buf[off:off + a.size]

    def step_fn(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, sqn, gs):
        n = p.size
        (pb, pv), (mb, mv), (vb, vv) = place(p, case.offset), place(m, 3 * case.offset), place(v, case.offset)
        assert pv.data_ptr() % 8 == 4 * case.offset
        tops.adam_step(pv, held['g'], mv, vv, lr, b1, b2, eps, wd, step, max_norm=max_norm, sqnorm=held['sq'] if sqn is not None else None,
                       grad_scale=gs)
        out = _host(pv), _host(mv), _host(vv)
        for buf, off in ((pb, case.offset), (mb, 3 * case.offset), (vb, case.offset)):
            assert _is_sent(buf[:off]) and _is_sent(buf[off + n:])
        return out

    return step_fn, sqnorm_fn


@pytest.mark.parametrize('n', tr.ADAM_NS)
@pytest.mark.parametrize('case_i', range(len(tr.ADAM_CASES)))
def test_adam_step_within_the_bounds(case_i, n):
    """param, exp_avg and exp_avg_sq after each of steps 1, 2, 3 carried on from the kernel's own state, and after one step at t = 100000"""
    case = tr.ADAM_CASES[case_i]
    for late in (False, True):
        step_fn, sqnorm_fn = _gpu_adam(case)
        for step, name, r in tr.adam_run(case_i, n, step_fn, sqnorm_fn, late=late):
            print('\nRATIO %-9s %-64s %.5f' % ('adam', '%s n=%d step %d %s' % (case.name, n, step, name), r))
            assert r <= 1.0, (case.name, n, step, name, r)


def test_adam_refuses_step_zero_and_a_null_state():
    lib, tops = _mods()
    L, p, st = lib.load(), tops._p, tops._stream()
    t = [_sent((64,)) for _ in range(4)]
    args = (64, 1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert L.pcp_adam_step(p(t[0]), p(t[1]), p(t[2]), p(t[3]), *args, 0, 0.0, None, 1.0, st) == ARG
    assert L.pcp_adam_step(p(t[0]), p(t[1]), None, p(t[3]), *args, 1, 0.0, None, 1.0, st) == ARG
    assert L.pcp_adam_step(p(t[0]), p(t[1]), p(t[2]), None, *args, 1, 0.0, None, 1.0, st) == ARG
    torch.cuda.synchronize()
    assert all(_is_sent(b) for b in t)
