"""Plain float64 references (numpy, no GPU, no torch) of the two kernel families every training iteration runs, the error bounds their
tests use as tolerance, and the case tables those tests share.

  bn_stats, scale_shift_act, bn_backward, colsum     csrc/bn_train.hip (k_col_reduce + the finalize kernels, k_scale_shift_act, k_bnbwd_apply)
  sqnorm, adam_step                                  csrc/optim.hip (k_sqnorm, k_adam)

Float32 and bf16 inputs enter the arithmetic as their exact float64 values; host scalars (eps, momentum, lr, ...) enter as the float32 the
C ABI passes.  Every reference returns its result next to the bound of every output, element by element, nothing on top.

Notation.  U = 2^-24 (one fp32 rounding, relative), U64 = 2^-53 (one float64 rounding), UB = 2^-8 (one bf16 rounding: 8 significand
bits, the hidden one included, so round-to-nearest-even of IO4<bf16_t>::st is within 2^-8 relative, not 2^-9).  to32(ref, e) =
e + U (|ref| + e): a value the kernel holds with error e in float64, then rounds to fp32.  A float64 sum of n exact terms t_i, added in
any order (per-thread partials, LDS tree, block partials, finalize), is within (n - 1) U64 sum |t_i| of the exact sum.  SECOND = 1 + 2^-20
covers the second-order terms (products of two of the errors below; every first-order sum here is below 2^-20).  Divide and sqrt are
correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), a contraction to FMA only removes roundings.

bn_stats (k_col_reduce<RED_STATS>, k_bn_finalize).  s0 = sum x and s1 = sum x^2 in float64 (the squares of floats are exact), n rows.
With A1 = sum |x| / n and A = sum x^2 / n:
    m = s0 / n                      dm   = n U64 A1                    (n - 1 additions and the division)
    var = s1 / n - m m              dvar = (3 n + 2) U64 A             (s1 / n: n U64 A.  m m: 2 |m| dm + U64 m^2 <= (2 n + 1) U64 A, as
                                                                        A1^2 <= A.  The subtraction: U64 var <= U64 A.)  This is the
                                                                        cancellation term of the one-pass form: relative to var it grows
                                                                        with A / var, and an fp32 accumulation (U in the place of U64) is
                                                                        2^29 times further out.  The clamp var >= 0 moves towards the truth.
    is = 1 / sqrt(var + eps)        dis  = is (rho / (2 (1 - rho)^1.5) + 3 U64), rho = dvar / (var + eps)   (mean value theorem on
                                                                        (1 - t)^-0.5; addition, sqrt, division round once each)
    scale = fl32(gamma is)          to32(., |gamma| dis + 2 U64 |scale|)
    shift = fl32(beta - m gamma is) to32(., |gamma| (|m| dis + is dm + dm dis) + 4 U64 (|beta| + |m gamma is|))
    mean = fl32(m), invstd = fl32(is)
    running_mean = fl32((1 - mom) rm + mom m)                           to32(., mom dm + 3 U64 (..))
    running_var  = fl32((1 - mom) rv + mom var n / (n - 1))             to32(., mom dvar n / (n - 1) + 4 U64 (..)); rows == 1 keeps the biased
                                                                        value (the kernel's rule: torch divides by zero there)

scale_shift_act (k_scale_shift_act): one fmaf, so |err| <= U |ref|; the clamp at 0 keeps it (a rounding never crosses zero, so the
output of a negative value is the reference's 0).  A bf16 output rounds once more: + UB (1 + U) |ref|.

bn_backward (k_col_reduce<RED_BNBWD>, k_bnbwd_finalize, k_bnbwd_apply), on the four fp32 vectors the kernel is given.
    act = fmaf(x, scale, shift); the mask is act > 0.  x scale is exact in float64 and adding shift keeps the sign of the exact value, a
    single rounding to fp32 keeps it too: the reference's float64 mask IS the kernel's, ties (act == 0) included, no slack.
    xh_k = fl(fl(x - mean) invstd) = xh (1 + 2 U)                       two roundings
    s0 = sum dz, s1 = sum dz xh_k in float64 (the products of two floats are exact).  With Tb = sum |dz|, Tg = sum |dz xh|:
    dbeta = fl32(s0)                to32(., n U64 Tb)
    dgamma = fl32(s1)               to32(., eg),  eg = (2 U + n U64) Tg
    c0 = fl32(s0 / n), c1 = fl32(s1 / n):  e0 = U |c0| + n U64 Tb / n,  e1 = U |c1| + eg / n
    dx = fl(scale fl(fl(dz - c0) - fl(xh_k c1))):  dz and c0 pass three roundings, xh c1 five (two in xh_k, the product, the
    subtraction, the scaling), so with S = |scale| (|dz| + |c0| + |xh c1|) split by term
    |err dx| <= |scale| (3 U |dz| + 3 U |c0| + e0 + |xh| (5 U |c1| + e1))
    A bf16 dx adds UB (|dx| + bound).  accumulate=1 adds the fp32 sums to what dgamma / dbeta held: accum_bound().
    The split (cross-rank) form reads the same sums: dgamma / dbeta from the shard's, c0 / c1 from the sums over all shards and the total
    row count, so dx meets the reference on the union and dgamma / dbeta the reference on the shard.

colsum: fl32 of a float64 sum: to32(., n U64 sum |x|).

sqnorm (k_sqnorm): squares (exact) and sums in float64, n non-negative terms in any order (grid stride, wave shuffles, atomics):
|err| <= n U64 ref.

adam_step (k_adam and the host scalars of pcp_adam_step).  The arithmetic, on float32 scalars:
    coef = grad_scale min(max_norm / (sqrt(sqnorm) |grad_scale| + 1e-6f), 1) with a sqnorm, grad_scale without
    decay = 1 - wd lr;  g' = g coef;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
    p' = p decay - lr / (1 - b1^t) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    coef: fl32(sqrt), the product with |grad_scale|, the addition, the division, the product with grad_scale: 5 U (min is 1-Lipschitz, so
          this also holds where kernel and reference fall on different sides of the threshold); exact without a sqnorm.  kc = 5 or 0.
    g':   (kc + 1) U = kg U
    m':   2 U |b1 m| + (kg + 3) U |(1 - b1) g'|                          (product and sum; fl(1 - b1), product, product, sum)
    v':   2 U b2 v + (2 kg + 4) U (1 - b2) g'^2
    D = sqrt(v') / sqrt(1 - b2^t) + eps:  dD = D1 (bv / (2 v') + 3 U) + U D  (half the relative error of v'; sqrtf, fl32(1 / sqrt(bc2)),
          the product; the addition)
    update = lr / bc1 m' / D:  bm lr / (bc1 D) + |update| (dD / D + 3 U)     (the division, fl32(lr / bc1), the product)
    p':   3 U |p decay| + [the update's] + U |update|                        (fl32(decay), the product, the final subtraction on both)
"""
import functools
from collections import namedtuple

import numpy as np

from pcp_amd import synth

U = 2.0 ** -24
U64 = 2.0 ** -53
UB = 2.0 ** -8
SECOND = 1.0 + 2.0 ** -20
TINY = 2.0 ** -149               # an fp32 result below the normal range rounds to within half of this


def f64(x):
    return np.asarray(x, dtype=np.float64)


def fl(v):
    """a host scalar as the C ABI passes it: rounded to float32"""
    return float(np.float32(v))


def to32(ref, e):
    return e + U * (np.abs(ref) + e) + TINY


def to_bf16(x):
    """float32 array rounded to the nearest bf16 (ties to even), returned as float32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((b + r) & np.uint32(0xffff0000)).view(np.float32)


def uniform(seed, col, shape, lo=-1.0, hi=1.0):
    n = int(np.prod(shape))
    return synth.uniform(9100 + seed, col, n, lo, hi).reshape(shape).astype(np.float32)


def accum_bound(parts, bounds):
    """fp32 sum of the values `parts` (first: what the buffer held, exact), each later one known within its entry of `bounds`: every
    addition rounds once, relative to a partial sum that is at most sum |parts| + sum bounds"""
    tot = sum(np.abs(f64(p)) for p in parts) + sum(bounds)
    return sum(bounds) + (len(parts) - 1) * U * tot


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm family
# ---------------------------------------------------------------------------------------------------------------------

def bn_stats(x, gamma, beta, eps, momentum, rm=None, rv=None):
    """x (rows, c).  -> dict: scale shift mean invstd [running_mean running_var] in float64, and 'b_' + name: the bound of the fp32 output"""
    x, g, b = f64(x), f64(gamma), f64(beta)
    eps, mom = fl(eps), fl(momentum)
    n = x.shape[0]
    m = x.sum(0) / n
    var = ((x - m) ** 2).sum(0) / n
    is_ = 1.0 / np.sqrt(var + eps)
    A1, A = np.abs(x).sum(0) / n, (x * x).sum(0) / n
    dm = n * U64 * A1
    dvar = (3 * n + 2) * U64 * A
    rho = dvar / (var + eps)
    assert (rho < 0.5).all(), 'the one-pass variance has no digits left at this offset'
    dis = is_ * (rho / (2 * (1 - rho) ** 1.5) + 3 * U64)
    scale, shift = g * is_, b - m * g * is_
    r = dict(scale=scale, shift=shift, mean=m, invstd=is_, var=var, dvar=dvar)
    r['b_scale'] = to32(scale, np.abs(g) * dis + 2 * U64 * np.abs(scale))
    r['b_shift'] = to32(shift, np.abs(g) * (np.abs(m) * dis + is_ * dm + dm * dis) + 4 * U64 * (np.abs(b) + np.abs(m * g * is_)))
    r['b_mean'] = to32(m, dm)
    r['b_invstd'] = to32(is_, dis)
    if rm is not None:
        rm, rv = f64(rm), f64(rv)
        fac = n / (n - 1.0) if n > 1 else 1.0
        r['running_mean'] = (1 - mom) * rm + mom * m
        r['running_var'] = (1 - mom) * rv + mom * var * fac
        r['b_running_mean'] = to32(r['running_mean'], mom * dm + 3 * U64 * (np.abs((1 - mom) * rm) + np.abs(mom * m)))
        r['b_running_var'] = to32(r['running_var'], mom * fac * dvar * SECOND + 4 * U64 * (np.abs((1 - mom) * rv) + mom * var * fac))
    return r


def vectors32(st):
    """the four vectors of a bn_stats result rounded to float32: what the backward kernel is handed"""
    return tuple(st[k].astype(np.float32) for k in ('scale', 'shift', 'mean', 'invstd'))


def scale_shift_act(x, scale, shift, relu, bf16_out=False):
    """-> (y, bound)"""
    y = f64(x) * f64(scale) + f64(shift)
    if relu:
        y = np.maximum(y, 0.0)
    bnd = U * np.abs(y) + TINY
    if bf16_out:
        bnd = bnd + UB * (1 + U) * np.abs(y)
    return y, bnd


def bn_backward(dout, x, scale, shift, mean, invstd, relu, bf16_dx=False):
    """-> dict: dgamma dbeta dx (float64), b_dgamma b_dbeta b_dx, masked (the count of elements the ReLU mask zeroes)"""
    d, x = f64(dout), f64(x)
    sc, sh, mu, is_ = f64(scale), f64(shift), f64(mean), f64(invstd)
    n = x.shape[0]
    if relu:
        keep = x * sc + sh > 0
        dz = np.where(keep, d, 0.0)
        masked = int(keep.size - keep.sum())
    else:
        dz, masked = d, 0
    xh = (x - mu) * is_
    dzxh = dz * xh
    Tb, Tg = np.abs(dz).sum(0), np.abs(dzxh).sum(0)
    dbeta, dgamma = dz.sum(0), dzxh.sum(0)
    eb = n * U64 * Tb
    eg = (2 * U * SECOND + n * U64) * Tg * SECOND
    c0, c1 = dbeta / n, dgamma / n
    e0 = U * np.abs(c0) + (eb + U64 * Tb) / n
    e1 = U * np.abs(c1) + (eg + U64 * Tg) / n
    dx = sc * (dz - c0 - xh * c1)
    b_dx = np.abs(sc) * (3 * U * np.abs(dz) + 3 * U * np.abs(c0) + e0 + np.abs(xh) * (5 * U * np.abs(c1) + e1)) * SECOND + TINY
    if bf16_dx:
        b_dx = b_dx + UB * (np.abs(dx) + b_dx)
    return dict(dgamma=dgamma, dbeta=dbeta, dx=dx, b_dgamma=to32(dgamma, eg), b_dbeta=to32(dbeta, eb), b_dx=b_dx, masked=masked)


def ratio(got, ref, bnd):
    """|got - ref| / bound, element by element; 0 where both are 0, inf where only the bound is"""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))


def worst(got, ref, bnd):
    """the largest ratio (nan when the output holds one: every comparison with it fails)"""
    r = ratio(got, ref, bnd)
    return float(r.max()) if r.size else 0.0


def colsum(x):
    """-> (sum over the rows, bound)"""
    x = f64(x)
    s = x.sum(0)
    return s, to32(s, x.shape[0] * U64 * np.abs(x).sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------

def sqnorm(g):
    """-> (sum g^2, bound)"""
    g = f64(g).reshape(-1)
    s = float((g * g).sum())
    return s, g.size * U64 * s * SECOND


def clip_coef(max_norm, sqn, grad_scale):
    gs = fl(grad_scale)
    if sqn is None:
        return gs, 0
    return gs * min(fl(max_norm) / (np.sqrt(float(sqn)) * abs(gs) + fl(1e-6)), 1.0), 5


def adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, max_norm=0.0, sqnorm=None, grad_scale=1.0):
    """-> dict: p m v (float64, after the step) and b_p b_m b_v"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    lr, b1, b2, eps, wd = fl(lr), fl(beta1), fl(beta2), fl(eps), fl(wd)
    coef, kc = clip_coef(max_norm, sqnorm, grad_scale)
    kg = kc + 1
    decay = 1.0 - wd * lr
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    gc = g * coef
    t_m0, t_m1 = b1 * m, (1 - b1) * gc
    t_v0, t_v1 = b2 * v, (1 - b2) * gc * gc
    m1, v1 = t_m0 + t_m1, t_v0 + t_v1
    b_m = (2 * U * np.abs(t_m0) + (kg + 3) * U * np.abs(t_m1)) * SECOND + TINY
    b_v = (2 * U * t_v0 + (2 * kg + 4) * U * t_v1) * SECOND + TINY
    D1 = np.sqrt(v1) / np.sqrt(bc2)
    D = D1 + eps
    with np.errstate(divide='ignore', invalid='ignore'):
        rv = np.where(v1 > 0, (b_v - TINY) / v1, 0.0)
    dD = D1 * (rv / 2 + 3 * U) + U * D
    ss = lr / bc1
    upd = ss * m1 / D
    pd = p * decay
    b_p = (3 * U * np.abs(pd) + ss * b_m / D + np.abs(upd) * (dD / D + 4 * U)) * SECOND + TINY
    return dict(p=pd - upd, m=m1, v=v1, b_p=b_p, b_m=b_m, b_v=b_v, coef=coef)


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every case names the code path it is there for
# ---------------------------------------------------------------------------------------------------------------------

RED_THREADS, RED_MAX_BLOCKS = 256, 512          # csrc/bn_train.hip
MOMENTUM = 0.01

BN = namedtuple('BN', 'rows c kind eps why')     # kind: 'uniform' x in [-2, 3] | 'offset' x = 100 + 0.01 u

BN_CASES = [
    BN(1, 4, 'uniform', 1e-3, 'single row, one column group'),
    BN(1, 64, 'uniform', 1e-3, 'single row: variance 0, the running variance keeps the biased value'),
    BN(7, 4, 'uniform', 1e-3, 'one column group, 256 row slots, fewer rows than slots'),
    BN(1000, 24, 'uniform', 1e-3, 'c / 4 = 6 does not divide 256: 4 idle threads'),
    BN(333, 48, 'uniform', 1e-3, 'c / 4 = 12: 4 idle threads, 21 row slots'),
    BN(3001, 32, 'uniform', 1e-3, 'the shape of the older test'),
    BN(9001, 384, 'uniform', 1e-3, 'block cap reached with 2 row slots'),
    BN(5000, 1024, 'uniform', 1e-3, '1 row slot, cap reached, unrolled loop plus tail'),
    BN(70001, 64, 'uniform', 1e-3, 'cap reached with 16 slots'),
    BN(4096, 64, 'offset', 1e-3, 'mean 100, deviation 0.006: pins the float64 sums'),
    BN(4096, 64, 'offset', 1e-5, 'the same with eps of the size of the variance'),
]
BN_TABLE = range(9)                              # the shape table proper; the offset cases follow
BN_WINDOW = (3, 4)                               # run once more as channel windows (ld = c + 16, ch_off = 8)
BN_STORAGE = BN(3000, 64, 'uniform', 1e-3, 'all eight storage-type combinations')
BN_SPLIT = BN(3001, 48, 'uniform', 1e-3, 'cross-rank split')
SPLITS = [(1, 3000), (1500, 1501)]
BN_TIES = BN(333, 48, 'ties', 1e-3, 'x scale + shift == 0 exactly at a tenth of the elements')
COLSUM_CASES = (0, 3, 7)


def red_plan(rows, c):
    """red_grid and the thread layout of k_col_reduce, restated: (row slots per block, blocks)"""
    rpb = RED_THREADS // (c // 4)
    return rpb, max(1, min(RED_MAX_BLOCKS, (rows + rpb * 8 - 1) // (rpb * 8)))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _bn_inputs(case, seed, bf16_x=False, bf16_dout=False):
    rows, c = case.rows, case.c
    if case.kind == 'offset':
        x = (100.0 + 0.01 * f64(uniform(seed, 1, (rows, c)))).astype(np.float32)
    else:
        x = uniform(seed, 1, (rows, c), -2.0, 3.0)
    dout = uniform(seed, 6, (rows, c))
    if bf16_x:
        x = to_bf16(x)
    if bf16_dout:
        dout = to_bf16(dout)
    return dict(x=x, dout=dout, gamma=uniform(seed, 2, (c,), 0.5, 1.5), beta=uniform(seed, 3, (c,), -0.2, 0.2),
                rm=uniform(seed, 4, (c,), -0.1, 0.1), rv=uniform(seed, 5, (c,), 0.5, 1.5))


def _bn_data(case, seed, **kw):
    d = _bn_inputs(case, seed, **kw)
    d['stats'] = _frozen(bn_stats(d['x'], d['gamma'], d['beta'], case.eps, MOMENTUM, d['rm'], d['rv']))
    d['vec'] = vectors32(d['stats'])
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def bn_data(i):
    """inputs (float32), the float64 statistics reference and its four vectors rounded to float32, of BN_CASES[i]; read-only"""
    return _bn_data(BN_CASES[i], 100 + i)


@functools.lru_cache(maxsize=None)
def split_data(bf16_x=False):
    return _bn_data(BN_SPLIT, 300, bf16_x=bf16_x)


@functools.lru_cache(maxsize=None)
def storage_data(bf16_x, bf16_dout):
    return _bn_data(BN_STORAGE, 200, bf16_x=bf16_x, bf16_dout=bf16_dout)


@functools.lru_cache(maxsize=4)
def bn_backward_data(i, relu):
    d = bn_data(i)
    return _frozen(bn_backward(d['dout'], d['x'], *d['vec'], relu))


@functools.lru_cache(maxsize=None)
def ties_data():
    """backward-only: scale 0.5, shift -1, x == 2 (activation exactly 0) at every tenth element, where dout is 1; x elsewhere in [-2, 6]"""
    rows, c = BN_TIES.rows, BN_TIES.c
    x = uniform(400, 1, (rows, c), -2.0, 6.0)
    dout = uniform(400, 6, (rows, c))
    tie = (np.arange(rows * c).reshape(rows, c) % 10) == 3
    x[tie], dout[tie] = 2.0, 1.0
    vec = (np.full(c, 0.5, np.float32), np.full(c, -1.0, np.float32), uniform(400, 7, (c,), 1.5, 2.5), uniform(400, 8, (c,), 0.4, 0.6))
    return _frozen(dict(x=x, dout=dout, tie=tie, vec=vec, ref=_frozen(bn_backward(dout, x, *vec, True))))


NORM_NS = [0, 1, 2, 3, 4, 5, 1023, 1310723]     # the last: 1.25 * 2^20 + 3, a second grid-stride trip for a quarter of the threads + a tail of 3


@functools.lru_cache(maxsize=None)
def norm_grad(n):
    g = uniform(500, n % 1000, (n,))
    g.setflags(write=False)
    return g


ADAM_NS = [1, 5, 257, 1310723]                  # 1310723 > 2048 * 256: a second and third trip of k_adam's grid-stride loop
BETA2, ADAM_EPS = 0.999, 1e-8

# clip: None (no sqnorm handed over) | ('rel', f): max_norm = f * |grad_scale| * norm (+ 1e-6 for f == 1) | ('abs', v)
Adam = namedtuple('Adam', 'name clip pass_sqnorm grad_scale wd gmag offset why')

ADAM_CASES = [
    Adam('clipped', ('rel', 0.5), True, 1.0, 0.01, 1.0, 0, 'norm at twice max_norm'),
    Adam('unclipped', ('rel', 2.0), True, 1.0, 0.01, 1.0, 0, 'norm at half max_norm: the coefficient clamps at 1'),
    Adam('threshold', ('rel', 1.0), True, 1.0, 0.01, 1.0, 0, 'max_norm = norm + 1e-6: the quotient is 1 to an ulp, either side'),
    Adam('no_sqnorm', ('abs', 1e-3), False, 1.0, 0.01, 1.0, 0, 'max_norm set, sqnorm=None: no clipping'),
    Adam('grad_scale', ('rel', 0.5), True, 0.125, 0.01, 1.0, 0, 'grad_scale 1/8, the norm taken on the unscaled buffer'),
    Adam('zero_grad', ('abs', 10.0), True, 1.0, 0.01, 0.0, 0, 'g = 0: a pure decay step, norm 0 under the 1e-6'),
    Adam('eps_dominates', None, False, 1.0, 0.01, 1e-12, 0, 'v = 0 and |g| ~ 1e-12: eps = 1e-8 is the denominator'),
    Adam('wd0', ('rel', 0.5), True, 1.0, 0.0, 1.0, 0, 'no weight decay: decay == 1'),
    Adam('odd_offset', ('rel', 0.5), True, 1.0, 0.01, 1.0, 1, 'param, exp_avg, exp_avg_sq at odd element offsets of larger buffers'),
]


def adam_hyper(step):
    """(lr, beta1) of a step: the one-cycle schedule moves both"""
    return 1e-3 * min(step, 3), 0.95 - 0.01 * min(step, 3)


def adam_grad(case_i, n, step):
    g = uniform(600 + case_i, 10 + step, (n,)) * np.float32(ADAM_CASES[case_i].gmag)
    return g.astype(np.float32)


def adam_param0(case_i, n):
    return uniform(600 + case_i, 1, (n,), -0.5, 0.5)


def adam_max_norm(case, sqn):
    """the float32 max_norm of a step whose unscaled gradient has the squared norm sqn"""
    if case.clip is None:
        return 0.0
    kind, val = case.clip
    if kind == 'abs':
        return fl(val)
    norm = np.sqrt(sqn) * abs(case.grad_scale)
    return fl(norm + 1e-6) if val == 1.0 else fl(val * norm)


def adam_late_state(n):
    """reference-made exp_avg / exp_avg_sq for the step at t = 100000"""
    return uniform(700, 1, (n,), -0.1, 0.1), uniform(700, 2, (n,), 0.0, 1e-2)


LATE_STEP = 100000


def adam_run(case_i, n, step_fn, sqnorm_fn, late=False):
    """Steps 1, 2, 3 of ADAM_CASES[case_i] on n parameters, every step carried on from what step_fn returned (late: the one step at
    LATE_STEP from adam_late_state).  step_fn(p, g, m, v, lr, beta1, beta2, eps, wd, step, max_norm, sqnorm | None, grad_scale) ->
    (p, m, v) float32; sqnorm_fn(g) -> the squared norm the step is handed.  -> [(step, 'p' | 'm' | 'v', worst ratio)]"""
    case = ADAM_CASES[case_i]
    p = adam_param0(case_i, n)
    m, v = adam_late_state(n) if late else (np.zeros(n, np.float32), np.zeros(n, np.float32))
    out = []
    for step in ((LATE_STEP,) if late else (1, 2, 3)):
        g = adam_grad(case_i, n, step)
        sqn = float(sqnorm_fn(g))
        lr, b1 = adam_hyper(step)
        args = (lr, b1, BETA2, ADAM_EPS, case.wd, step, adam_max_norm(case, sqn), sqn if case.pass_sqnorm else None, case.grad_scale)
        ref = adam_step(p, g, m, v, *args)
        p, m, v = step_fn(p, g, m, v, *args)
        for name, got in (('p', p), ('m', m), ('v', v)):
            out.append((step, name, worst(got, ref[name], ref['b_' + name])))
    return out
