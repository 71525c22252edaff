"""The float64 references, bounds and case tables of tests/train_step_refs.py, checked on the CPU: the references against torch's own float64
BatchNorm / autograd and torch.optim.Adam, the bounds against an fp32 numpy emulation of each kernel's arithmetic that sums in another
order than the kernel (it has to stay inside every bound of every case the GPU tests run), and against eleven deliberate faults, each
of which has to leave a bound on at least one of those cases.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_step_refs as tr

F32 = np.float32
BN_IDS = range(len(tr.BN_CASES))
BY_SIZE = sorted(BN_IDS, key=lambda i: tr.BN_CASES[i].rows * tr.BN_CASES[i].c)      # the fault tests stop at the first case that shows it


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _rel(got, want):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(1e-300, np.abs(want).max()))


# ---- the references against torch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i,relu', [(1, True), (2, False), (4, True), (5, True), (5, False), (9, True)])
def test_bn_references_equal_torch_batch_norm_and_autograd_in_float64(i, relu):
    c, d = tr.BN_CASES[i], tr.bn_data(i)
    x = _t(d['x']).requires_grad_(True)
    g, b = _t(d['gamma']).requires_grad_(True), _t(d['beta']).requires_grad_(True)
    rm, rv = _t(d['rm']), _t(d['rv'])
    if c.rows == 1:                      # torch refuses one value per channel in training mode: the batch statistics from their definition
        y = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + tr.fl(c.eps)) * g + b
        rm = (1 - tr.fl(tr.MOMENTUM)) * rm + tr.fl(tr.MOMENTUM) * x.detach().mean(0)
        rv = (1 - tr.fl(tr.MOMENTUM)) * rv + tr.fl(tr.MOMENTUM) * x.detach().var(0, unbiased=False)     # the kernel's rule
    else:
        y = F.batch_norm(x, rm, rv, g, b, training=True, momentum=tr.fl(tr.MOMENTUM), eps=tr.fl(c.eps))
    y = y.clamp_min(0) if relu else y
    y.backward(_t(d['dout']))
    st = d['stats']
    out, _b = tr.scale_shift_act(d['x'], st['scale'], st['shift'], relu)
    tol = 1e-12 if c.kind == 'uniform' else 1e-7          # the offset case: torch's own float64 statistics carry the cancellation
    assert _rel(out, y) <= tol
    assert _rel(st['running_mean'], rm) <= tol and _rel(st['running_var'], rv) <= tol
    bw = tr.bn_backward(d['dout'], d['x'], st['scale'], st['shift'], st['mean'], st['invstd'], relu)
    assert _rel(bw['dgamma'], g.grad) <= tol and _rel(bw['dbeta'], b.grad) <= tol and _rel(bw['dx'], x.grad) <= tol


def test_colsum_and_sqnorm_references():
    x = tr.bn_data(4)['x']
    s, b = tr.colsum(x)
    assert _rel(s, _t(x).sum(0)) <= 1e-14 and (b > 0).all()
    g = tr.norm_grad(1023)
    s, b = tr.sqnorm(g)
    assert abs(s - float(_t(g).norm() ** 2)) <= 1e-13 * s and 0 < b < 1e-12 * s


@pytest.mark.parametrize('case_i', range(len(tr.ADAM_CASES)))
def test_adam_reference_equals_torch_adam_in_float64(case_i):
    """clip_grad_norm_, the p.mul_(1 - wd lr) pre-step and torch.optim.Adam on a float64 parameter, three steps"""
    case, n = tr.ADAM_CASES[case_i], 257
    ref = _t(tr.adam_param0(case_i, n)).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=0.0, betas=(0.9, tr.fl(tr.BETA2)), eps=tr.fl(tr.ADAM_EPS))
    state = {}

    def torch_step(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, sqn, gs):
        ref.grad = _t(g) * tr.fl(gs)
        if sqn is not None:
            torch.nn.utils.clip_grad_norm_([ref], tr.fl(max_norm))
        for grp in opt.param_groups:
            grp['lr'], grp['betas'] = tr.fl(lr), (tr.fl(b1), tr.fl(b2))
        with torch.no_grad():
            ref.mul_(1 - tr.fl(wd) * tr.fl(lr))
        opt.step()
        st = opt.state[ref]
        state['got'] = (ref.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy())
        mine = tr.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, sqn, gs)
        for k, want in zip('pmv', state['got']):
            assert _rel(mine[k], want) <= 1e-12, (case.name, step, k)
        return state['got']                 # float64 carried on: both sides see the same state

    tr.adam_run(case_i, n, torch_step, lambda g: tr.sqnorm(g)[0])


# ---- fp32 emulations of the kernels' arithmetic, summing in another order; `wrong` names one deliberate fault ----------------------------

def emu_stats(x, gamma, beta, eps, momentum, rm, rv, wrong=None):
    x = np.asarray(x, F32)
    n = x.shape[0]
    if wrong == 'fp32_sums':
        s0, s1 = tr.f64(x.sum(0, dtype=F32)), tr.f64((x * x).sum(0, dtype=F32))
    else:                                   # last row first, one after the other (the kernel: strided per-thread partials, then trees)
        x64 = tr.f64(x)[::-1]
        s0, s1 = x64.sum(0), (x64 * x64).sum(0)
    eps, mom = tr.fl(eps), tr.fl(momentum)
    m = s0 / n
    var = np.maximum(s1 / n - m * m, 0.0)
    unb = var * n / (n - 1.0) if n > 1 else var
    is_ = 1.0 / np.sqrt((unb if wrong == 'unbiased_invstd' else var) + eps)
    g, b = tr.f64(gamma), tr.f64(beta)
    out = dict(scale=g * is_, shift=b - m * g * is_, mean=m, invstd=is_,
               running_mean=(1 - mom) * tr.f64(rm) + mom * m,
               running_var=(1 - mom) * tr.f64(rv) + mom * (var if wrong == 'biased_running_var' else unb))
    return {k: v.astype(F32) for k, v in out.items()}


def emu_backward(dout, x, scale, shift, mean, invstd, relu, wrong=None):
    d, x = np.asarray(dout, F32), np.asarray(x, F32)
    sc, sh, mu, is_ = (np.asarray(v, F32) for v in (scale, shift, mean, invstd))
    n = x.shape[0]
    dz = d
    if relu:
        act = tr.f64(x) * tr.f64(sc) + tr.f64(sh)            # fmaf: the sign of the exact value
        dz = np.where(act >= 0 if wrong == 'mask_ge' else act > 0, d, F32(0))
    xh = (x - mu) * is_
    s0, s1 = tr.f64(dz)[::-1].sum(0), (tr.f64(dz) * tr.f64(xh))[::-1].sum(0)
    c0, c1 = (s0 / n).astype(F32), (s1 / n).astype(F32)
    t = dz - c0
    dx = sc * (t if wrong == 'no_c1' else t - xh * c1)
    assert dx.dtype == F32
    return dict(dgamma=s1.astype(F32), dbeta=s0.astype(F32), dx=dx)


def emu_sqnorm(g, wrong=None):
    g = tr.f64(np.asarray(g, F32))
    if wrong == 'no_tail':
        g = g[:g.size & ~3]
    return float((g * g)[::-1].sum())


def emu_adam(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, sqn, gs, wrong=None):
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, max_norm, gs = (F32(a) for a in (lr, b1, b2, eps, wd, max_norm, gs))
    coef = gs
    if sqn is not None:
        norm = F32(np.sqrt(sqn))
        if wrong != 'no_grad_scale_in_norm':
            norm = norm * abs(gs)
        c = max_norm / (norm + F32(1e-6))
        coef = coef * (c if wrong == 'no_clamp' else min(c, F32(1)))
    decay = F32(1) if wrong == 'no_weight_decay' else F32(1.0 - float(wd) * float(lr))
    t = step - 1 if wrong == 'step_minus_1' and step > 1 else step
    step_size = F32(float(lr) / (1.0 - float(b1) ** t))
    inv_sqrt_bc2 = F32(1.0 / np.sqrt(1.0 - float(b2) ** t))
    gc = g * coef
    m1 = b1 * m + (F32(1) - b1) * gc
    v1 = b2 * v + (F32(1) - b2) * gc * gc
    if wrong == 'eps_in_sqrt':
        denom = np.sqrt(v1 * inv_sqrt_bc2 * inv_sqrt_bc2 + eps)
    else:
        denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
    p1 = p * decay - step_size * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == F32
    return p1, m1, v1


def stats_ratios(d, case, wrong=None):
    st = d['stats']
    got = emu_stats(d['x'], d['gamma'], d['beta'], case.eps, tr.MOMENTUM, d['rm'], d['rv'], wrong)
    return {k: tr.worst(got[k], st[k], st['b_' + k]) for k in got}


def backward_ratios(d, ref, relu, wrong=None, bf16_dx=False):
    got = emu_backward(d['dout'], d['x'], *d['vec'], relu, wrong)
    if bf16_dx:
        got['dx'] = tr.to_bf16(got['dx'])
    return {k: tr.worst(got[k], ref[k], ref['b_' + k]) for k in got}


def _inside(ratios, what):
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


def _outside(ratios, keys):
    return any(not ratios[k] <= 1.0 for k in keys)


# ---- a correct emulation stays inside every bound of every GPU case ----------------------------------------------------------------------

@pytest.mark.parametrize('i', BN_IDS)
def test_bn_emulation_is_inside_the_bounds(i):
    case, d = tr.BN_CASES[i], tr.bn_data(i)
    _inside(stats_ratios(d, case), 'stats')
    v = emu_stats(d['x'], d['gamma'], d['beta'], case.eps, tr.MOMENTUM, d['rm'], d['rv'])
    for relu in (False, True):
        y, b = tr.scale_shift_act(d['x'], v['scale'], v['shift'], relu)          # on the emulation's own vectors, as on the GPU
        got = np.asarray(tr.f64(d['x']) * tr.f64(v['scale']) + tr.f64(v['shift']), F32)   # exact, then one rounding: fmaf
        got = np.maximum(got, F32(0)) if relu else got
        assert tr.worst(got, y, b) <= 1.0
        _inside(backward_ratios(d, tr.bn_backward_data(i, relu), relu), 'backward relu=%d' % relu)


def test_tables_reach_the_paths_they_name():
    plans = [tr.red_plan(c.rows, c.c) for c in tr.BN_CASES]
    assert plans[2] == (256, 1) and plans[3][0] * 6 == 252 and plans[4][0] * 12 == 252
    assert plans[6] == (2, 512) and plans[7] == (1, 512) and plans[8] == (16, 512)
    assert 5000 > 4 * 512 and 5000 % (4 * 512) != 0                              # unrolled trips and a tail at one row slot
    assert all(tr.red_plan(c.rows, c.c)[1] < 512 for c in tr.BN_CASES[:6])
    n = tr.NORM_NS[-1]
    assert n == 5 * 2 ** 18 + 3 and n // 4 > 1024 * 256 and n > 2048 * 256 and n & 3 == 3
    t = tr.ties_data()
    assert t['tie'].sum() > 1000 and (tr.f64(t['x'][t['tie']]) * 0.5 - 1.0 == 0).all() and t['ref']['masked'] > t['tie'].sum()


def test_ties_storage_and_split_emulations_are_inside_the_bounds():
    t = tr.ties_data()
    _inside(backward_ratios(t, t['ref'], True), 'ties')
    for bx in (False, True):
        _inside(stats_ratios(tr.storage_data(bx, False), tr.BN_STORAGE), 'storage stats')
        for bd in (False, True):
            d = tr.storage_data(bx, bd)
            for bo in (False, True):
                _inside(backward_ratios(d, tr.bn_backward(d['dout'], d['x'], *d['vec'], True, bf16_dx=bo), True, bf16_dx=bo), (bx, bd, bo))
    d = tr.split_data()
    _inside(stats_ratios(d, tr.BN_SPLIT), 'split stats')
    _inside(backward_ratios(d, tr.bn_backward(d['dout'], d['x'], *d['vec'], True), True), 'split backward')


@pytest.mark.parametrize('n', tr.NORM_NS)
def test_sqnorm_emulation_is_inside_the_bound(n):
    s, b = tr.sqnorm(tr.norm_grad(n))
    assert abs(emu_sqnorm(tr.norm_grad(n)) - s) <= b


@pytest.mark.parametrize('n', tr.ADAM_NS)
@pytest.mark.parametrize('case_i', range(len(tr.ADAM_CASES)))
def test_adam_emulation_is_inside_the_bounds(case_i, n):
    for late in (False, True):
        for step, name, r in tr.adam_run(case_i, n, emu_adam, emu_sqnorm, late=late):
            assert r <= 1.0, (tr.ADAM_CASES[case_i].name, n, step, name, r)


# ---- every deliberate fault leaves a bound on at least one case ---------------------------------------------------------------------------

def test_fault_statistics_accumulated_in_fp32():
    assert any(_outside(stats_ratios(tr.bn_data(i), tr.BN_CASES[i], 'fp32_sums'), ('scale', 'shift', 'invstd')) for i in BY_SIZE)
    # and it is the offset cases that show it where the older range [-2, 3] does not have to
    assert all(_outside(stats_ratios(tr.bn_data(i), tr.BN_CASES[i], 'fp32_sums'), ('invstd',)) for i in (9, 10))


def test_fault_unbiased_variance_in_invstd():
    assert any(_outside(stats_ratios(tr.bn_data(i), tr.BN_CASES[i], 'unbiased_invstd'), ('scale', 'invstd')) for i in BY_SIZE)


def test_fault_running_variance_from_the_biased_value():
    assert any(_outside(stats_ratios(tr.bn_data(i), tr.BN_CASES[i], 'biased_running_var'), ('running_var',)) for i in BY_SIZE)


def test_fault_relu_mask_greater_or_equal():
    t = tr.ties_data()
    r = backward_ratios(t, t['ref'], True, 'mask_ge')
    assert not r['dgamma'] <= 1.0 and not r['dbeta'] <= 1.0 and not r['dx'] <= 1.0, r


def test_fault_dx_without_the_xhat_term():
    assert any(_outside(backward_ratios(tr.bn_data(i), tr.bn_backward_data(i, True), True, 'no_c1'), ('dx',)) for i in BY_SIZE)


def _adam_fault(wrong, case_names, ns=tr.ADAM_NS[:3]):
    def step(*a):
        return emu_adam(*a, wrong=wrong)
    for case_i, case in enumerate(tr.ADAM_CASES):
        if case.name in case_names:
            for n in ns:
                if any(not r <= 1.0 for _s, _n, r in tr.adam_run(case_i, n, step, emu_sqnorm)):
                    return True
    return False


ALL_ADAM = tuple(c.name for c in tr.ADAM_CASES)


def test_fault_bias_correction_with_step_minus_1():
    assert _adam_fault('step_minus_1', ALL_ADAM)


def test_fault_eps_inside_the_sqrt():
    assert _adam_fault('eps_in_sqrt', ALL_ADAM)
    assert _adam_fault('eps_in_sqrt', ('eps_dominates',))


def test_fault_weight_decay_dropped():
    assert _adam_fault('no_weight_decay', ALL_ADAM)
    assert not _adam_fault('no_weight_decay', ('wd0',))          # and the bound is what sees it: without decay there is nothing to see


def test_fault_clip_coefficient_not_clamped():
    assert _adam_fault('no_clamp', ('unclipped',))
    assert not _adam_fault('no_clamp', ('clipped',))


def test_fault_grad_scale_left_out_of_the_norm():
    assert _adam_fault('no_grad_scale_in_norm', ('grad_scale',))
    assert not _adam_fault('no_grad_scale_in_norm', ('clipped',))


def test_fault_tail_left_out_of_the_norm():
    bad = [n for n in tr.NORM_NS if not abs(emu_sqnorm(tr.norm_grad(n), 'no_tail') - tr.sqnorm(tr.norm_grad(n))[0]) <= tr.sqnorm(tr.norm_grad(n))[1]]
    assert bad == [n for n in tr.NORM_NS if n & 3], bad
