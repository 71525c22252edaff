"""Plain float64 references (numpy, no GPU, no torch) of the dense-head and distillation loss kernels, the error bounds their tests use
as tolerance, and the case tables those tests share.

  centerhead_loss        csrc/loss.hip (k_focal_reduce, k_reg_reduce, k_headloss_finalize, k_focal_grad, k_reg_grad)
  centerhead_loss_ext    csrc/loss.hip (k_lossx_reduce, k_lossx_finalize, k_lossx_focal_grad, k_lossx_reg_grad)
  anchor_loss            csrc/anchor_train.hip (k_count_positives, k_anchor_loss, k_anchor_loss_finalize)
  distill_loss           csrc/loss.hip (k_distill, k_distill_finalize)

Float32 inputs enter the arithmetic as their exact float64 values; host scalars (weights, grad_scale, dir_offset, ...) enter as the float32
the C ABI passes.  Every reference returns its result next to the bound of every output, element by element, nothing on top.  U, U64, the
float64-sum rule (n terms added in any order are within n U64 sum |t_i| of their sum) and ratio() / worst() are train_step_refs's.

How a bound is derived.  Each kernel's expression is evaluated once more, operation by operation and in the kernel's own order
(#pragma clang fp contract(off): no FMA), on pairs V(v, e): v the float64 value of the exact expression, e a bound of |what the kernel
holds - v|.  The rules, with |x| the magnitude of the float64 value and ^ the carried bound:
    a + b, a - b        e = ea + eb
    a b                 e = |a| eb + |b| ea + ea eb
    a / b               e = (ea + |a / b| eb) / (|b| - eb)                              (|b| > eb is asserted)
    expf(a)             e = exp(a) (exp(ea) - 1)          then EXP_ULP ulp of the result
    logf(a)             e = -log(1 - ea / a)              then LOG_ULP ulp              (a > ea is asserted)
    log1pf(a)           e = -log(1 - ea / (1 + a))        then LOG1P_ULP ulp
    sinf(a), cosf(a)    e = ea                            then SINCOS_ULP ulp
    one rounding of unit u (U for an fp32 operation, U64 for a float64 one, U for a cast double -> float):
                        e += u (|v| + e) + FLUSH          FLUSH = 2^-126 for fp32: a result below the normal range, kept or flushed
Every fp32 operation of the kernel counts as one rounding, the exact ones (1 - p for p >= 1/2, a product with 0, 1 or 0.25) included: the
bound only grows by that.  Nothing is linearised, so no second-order factor is needed.  k ulp of a result r are at most k 2^-23 |r|.

The transcendental functions are the only numbers that do not follow from the source.  EXP_ULP = 3, LOG_ULP = 3, LOG1P_ULP = 2,
SINCOS_ULP = 4: the maximum errors the OpenCL full profile allows for exp, log, log1p, sin and cos (OpenCL C specification, "Relative
error as ULPs"), which the OCML device library behind HIP's expf / logf / log1pf / sinf / cosf is built to meet.  The ROCm installation
ships that library as bitcode only, with no document of tighter figures for the HIP device functions, so these stand.

Sums.  A float64 sum (focal sums, L1 sums, the loss sums of k_anchor_loss and k_distill) of n fp32 terms t_i, each held within e_i:
sum e_i + n U64 sum (|t_i| + e_i), whatever the order (grid stride, wave shuffles, LDS, atomics or fixed-order block partials).  An fp32
sum of n terms in any order (the atomics of k_reg_grad over the slots of a cell, the slot-order sum of k_lossx_reg_grad):
sum e_i + (n - 1) U sum (|t_i| + e_i): n - 1 additions, every partial sum at most sum |t_i|; the first addition to the zero the dense
kernel stored is exact.  An fp32 sum by a tree of known shape, in which no term passes through more than D additions:
sum e_i + ((1 + U)^D - 1) sum (|t_i| + e_i).  k_distill adds the 8 values of a lane one after the other onto a zero (7 roundings), then
runs six butterfly steps over the 64 lanes: D = 13 for sf, se and dot, whatever c; the direction softmax of k_anchor_loss adds its bins
one after the other: D = bins - 1.

Discontinuities are designed out of the inputs (the generators below, asserted by tests/test_loss_refs_cpu.py for every case), never
masked out of a comparison:
    clamped sigmoid     s = 1 / (1 + expf(-x)), inside = LO <= s <= HI, p = clamp(s): a logit is at least CLAMP_MARGIN = 2^-5 away from
                        logit(LO) and logit(HI) (the generators plant logits at 1.25 margins on both sides of both, and at +-12, +-30).
                        At HI, the narrow side, the margin moves s by HI (1 - HI) 2^-5 = 3.1e-6, 25 times the 1.2e-7 the three roundings of
                        s can be off; so kernel and reference agree on `inside`, and an outside p is LO or HI exactly
    sign of an L1 difference (CenterHead)   head - target is 0 exactly (the same float32) or at least L1_MARGIN = 2^-10; fl(a - b) has the
                        sign of a - b anyway, the margin keeps |diff| far from the relative error of its own rounding
    direction bin       q = limit_period(target + anchor heading - dir_offset) / dir_period is at least DIR_MARGIN = 2^-8 from an integer
                        (fp32 evaluation moves q by less than 2^-16 at these magnitudes), wraps below 0 and at or above 2 pi included: a
                        wrap edge is a bin edge, so the same margin covers floorf(v / two_pi)
    smooth L1 (anchor)  value and slope are continuous at |d| = beta; where the reference's |d| is within its own error of beta the other
                        branch differs by (|d| - beta)^2 / (2 beta) in value and | |d| - beta | / beta in slope, which is added there.
                        Its sign(d) branch only runs for |d| >= beta = 1/9.  Distillation: |softmax difference| < 1 always.

centerhead_loss.  Per heat-map element: p = clamp(s); gt == 1: t = (logf(p) (1 - p)) (1 - p); gt < 1: w = (1 - gt) (1 - gt),
t = ((logf(1 - p) p) p) (w w).  pos, neg: float64 sums.  hm = cls_weight * (num_pos == 0 ? -neg : -(pos + neg) / num_pos) in float64, cast.
Per code j: S_j = float64 sum of |fl(head - target)| over the valid slots whose target is not NaN; loc = loc_weight sum_j
code_weight_j (float)(S_j / max(mask sum, 1)) in float64, cast; losses[2] = (float)(hm + loc) from the float64 values.  Gradient of a
heat-map channel: coef = (-cls_weight grad_scale) / (float)max(num_pos, 1); dldp = ((1 - p)(1 - p)) / p - (2 (1 - p)) logf(p) at a
positive (0 when num_pos == 0), (w w)((-(p p)) / (1 - p) + (2 p) logf(1 - p)) at a negative; g = ((coef dldp) p)(1 - p) inside the clamp,
0 exactly outside.  Gradient of a regression channel at a cell: the fp32 sum over its slots of
(((sign loc_weight) code_weight_j) grad_scale) / (float)num.  Every other channel below ld_d: 0 exactly.

centerhead_loss_ext: the same arithmetic per head with n_codes codes and no NaN skip (targets are finite by contract); total = the fp32
sum, in head order, of the float32 losses[h][2].

anchor_loss.  norm_b = max(positives of frame b, 1) (exact), w = 1 / norm_b, inv_b = 1 / batch.  Class logit x with one-hot t:
p = 1 / (1 + expf(-x)), aw = 0.25 t + 0.75 (1 - t), pt = t (1 - p) + (1 - t) p, bce = (max(x, 0) - x t) + log1pf(expf(-|x|)),
term = ((aw (pt pt)) bce) w (label -1: w = 0), g = ((((aw (((2 pt) dpt) bce + (pt pt)(p - t))) w) cls_weight) inv_b) grad_scale with
dpt = ((1 - 2 t) p)(1 - p).  Box code j of a positive with a target that is not NaN: d = (pred - target) cw_j, for the heading
d = (sinf(pred) cosf(target) - cosf(pred) sinf(target)) cw_6 and chain = cosf cosf + sinf sinf; term = smooth_l1(d, beta = 1/9) w,
g = (((((ds cw_j) chain) w) loc_weight) inv_b) grad_scale.  Direction of a positive: lse = mx + logf(sum_k expf(x_k - mx)) (sequential
fp32 sum), term = (lse - x_bin) w, g_k = ((((expf(x_k - lse) - [k == bin]) w) dir_weight) inv_b) grad_scale.  The three sums are float64;
loss = sum / batch * weight in float64, cast; losses[3] = (float)(cls + loc + dir); losses[4] = positives of the batch.

distill_loss.  Per pixel: F_i = expf(fl(f_i - max f)), sf = fp32 sum, a_i = F_i / sf; the same for early giving b_i; d_i = a_i - b_i;
term = (0.5 d_i) d_i, float64 sum; loss = (float)(sum / (pixels c) * weight).  dot = fp32 sum of d_i a_i;
g_i = ((k a_i)(d_i - dot)), k = (weight grad_scale) (float)(1 / (pixels c)); accumulate adds g to the prior with one more rounding.
"""
import functools
from collections import namedtuple

import numpy as np

from train_step_refs import U, U64, f64, fl, ratio, worst          # noqa: F401  (ratio, worst: re-exported for the tests)

ULP = 2.0 ** -23                 # k ulp of a normal fp32 result r are at most k ULP |r|
FLUSH = 2.0 ** -126              # an fp32 result below the normal range, kept as a subnormal or flushed to zero
EXP_ULP, LOG_ULP, LOG1P_ULP, SINCOS_ULP = 3, 3, 2, 4       # OpenCL C specification, full profile: exp, log, log1p, sin / cos
F32 = np.float32
LO = float(F32(1e-4))                                     # the clamp of clamped_sigmoid, as the compiler folds `1e-4f`, `1.f - 1e-4f`
HI = float(F32(1.0) - F32(1e-4))
X_LO, X_HI = float(np.log(LO / (1 - LO))), float(np.log(HI / (1 - HI)))      # the logits whose sigmoid is LO, HI
CLAMP_MARGIN = 2.0 ** -5
L1_MARGIN = 2.0 ** -10
DIR_MARGIN = 2.0 ** -8
BETA = float(F32(1.0) / F32(9.0))
TWO_PI32 = float(F32(6.283185307179586))
LX_STRIDE = 64 * 256             # LX_BLOCKS * 256 of k_lossx_reduce
FOCAL_SWEEP = 1024 * 256         # the block cap of pcp_centerhead_loss times the block size: one sweep of k_focal_reduce
MAX_HEADS, MAX_CODES = 8, 16     # PCP_DET_MAX_HEADS, PCP_HEADLOSS_MAX_CODES (the GPU test asserts both against the header)


# ---------------------------------------------------------------------------------------------------------------------
# values with an error bound
# ---------------------------------------------------------------------------------------------------------------------

class V:
    """v: the float64 value of the exact expression; e: a bound of |what the kernel holds - v|"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v = f64(v)
        self.e = np.broadcast_to(f64(e), self.v.shape) if np.ndim(e) == 0 else f64(e)

    def __getitem__(self, k):
        return V(self.v[k], np.broadcast_to(self.e, self.v.shape)[k])


def lift(x):
    return x if isinstance(x, V) else V(x)


def rnd(v, e, u):
    return V(v, e + u * (np.abs(v) + e) + (FLUSH if u == U else 0.0)) if u else V(v, e)


def add(a, b, u=U):
    a, b = lift(a), lift(b)
    return rnd(a.v + b.v, a.e + b.e, u)


def sub(a, b, u=U):
    a, b = lift(a), lift(b)
    return rnd(a.v - b.v, a.e + b.e, u)


def mul(a, b, u=U):
    a, b = lift(a), lift(b)
    return rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, u)


def div(a, b, u=U):
    a, b = lift(a), lift(b)
    assert (np.abs(b.v) > b.e).all(), 'a divisor that may be zero'
    q = a.v / b.v
    return rnd(q, (a.e + np.abs(q) * b.e) / (np.abs(b.v) - b.e), u)


def neg(a):
    return V(-a.v, a.e)


def vabs(a):
    return V(np.abs(a.v), a.e)


def cast32(a):
    """double -> float"""
    return rnd(a.v, a.e, U)


def _ulps(v, e, k):
    return V(v, e + k * ULP * (np.abs(v) + e) + FLUSH)


def vexp(a):
    a = lift(a)
    v = np.exp(a.v)
    return _ulps(v, v * np.expm1(a.e), EXP_ULP)


def vlog(a):
    a = lift(a)
    assert (a.v > a.e).all(), 'the logarithm of a value that may be zero'
    return _ulps(np.log(a.v), -np.log1p(-a.e / a.v), LOG_ULP)


def vlog1p(a):
    a = lift(a)
    assert (1.0 + a.v > a.e).all()
    return _ulps(np.log1p(a.v), -np.log1p(-a.e / (1.0 + a.v)), LOG1P_ULP)


def vsin(a):
    a = lift(a)
    return _ulps(np.sin(a.v), a.e, SINCOS_ULP)


def vcos(a):
    a = lift(a)
    return _ulps(np.cos(a.v), a.e, SINCOS_ULP)


def where(c, a, b):
    a, b = lift(a), lift(b)
    return V(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def dsum(t, mask=None, axis=None):
    """float64 sum of the fp32 terms t (those of mask), any order"""
    m = np.ones(t.v.shape, bool) if mask is None else mask
    v, e = np.where(m, t.v, 0.0), np.where(m, t.e, 0.0)
    n = m.sum(axis=axis)
    return V(v.sum(axis=axis), e.sum(axis=axis) + n * U64 * (np.abs(v) + e).sum(axis=axis))


def fsum(t, axis, depth):
    """fp32 sum of the terms t along an axis by a tree in which no term passes through more than `depth` additions"""
    tot = (np.abs(t.v) + t.e).sum(axis=axis)
    return V(t.v.sum(axis=axis), t.e.sum(axis=axis) + ((1.0 + U) ** depth - 1.0) * tot + FLUSH)


DIST_DEPTH = 7 + 6               # k_distill: DIST_MAXV = 8 terms per lane onto a zero (the first addition is exact), six butterfly steps


ONE = V(1.0)


def sigmoid(x):
    """1.f / (1.f + expf(-x))"""
    return div(ONE, add(ONE, vexp(V(-f64(x)))))


def clamped_sigmoid(x):
    """-> (p, inside, s): the margins of the generators make `inside` the kernel's, and an outside p exact"""
    s = sigmoid(x)
    inside = (s.v >= LO) & (s.v <= HI)
    return V(np.clip(s.v, LO, HI), np.where(inside, s.e, 0.0)), inside, s


# ---------------------------------------------------------------------------------------------------------------------
# CenterHead
# ---------------------------------------------------------------------------------------------------------------------

def _focal(x, gt, cls_weight, grad_scale, fault=None):
    """x, gt: the logits and the heat map, same shape.  -> (hm loss V in float64 before the cast, num_pos, gradient V)"""
    gt = f64(gt)
    p, inside, _s = clamped_sigmoid(x)
    q = sub(ONE, p)
    ispos, isneg = gt == 1.0, gt < 1.0
    w = sub(ONE, V(gt))
    w = mul(w, w)
    w4 = w if fault == 'neg_exp2' else mul(w, w)
    t_pos = mul(mul(vlog(p), q), q)
    t_neg = mul(mul(mul(vlog(q), p), p), w4)
    if fault == 'fp32_sum':                                  # one fp32 accumulator, element order
        def s32(t, m):
            acc = F32(0)
            for val in np.where(m, t.v, 0.0).astype(F32).reshape(-1):
                acc = F32(acc + val)
            return V(float(acc))
        pos, negs = s32(t_pos, ispos), s32(t_neg, isneg)
    else:
        pos, negs = dsum(t_pos, ispos), dsum(t_neg, isneg)
    npos = int(ispos.sum())
    hm = neg(negs) if npos == 0 else div(neg(add(pos, negs, U64)), float(npos), U64)
    hm = mul(hm, cls_weight, U64)
    coef = div(mul(-cls_weight, grad_scale), float(max(npos, 1)))
    d_pos = sub(div(mul(q, q), p), mul(mul(2.0, q), vlog(p)))
    if npos == 0:
        d_pos = V(np.zeros_like(gt))
    d_neg = mul(w4, add(div(neg(mul(p, p)), q), mul(mul(2.0, p), vlog(q))))
    dldp = where(ispos, d_pos, where(isneg, d_neg, V(np.zeros_like(gt))))
    g = mul(mul(mul(coef, dldp), p), q)
    if fault != 'no_clamp_zero':
        g = where(inside, g, V(np.zeros_like(gt)))
    return hm, npos, g


def _reg(head, tb, inds, mask, reg_ch, code_weights, loc_weight, grad_scale, ld_d, skip_nan, fault=None):
    """head (B, HW, ld).  -> (loc loss V in float64 before the cast, gradient value (B, HW, ld_d), its bound)"""
    B, HW, _ld = head.shape
    nc = len(reg_ch)
    head, tb = f64(head), f64(tb)
    valid = np.asarray(mask) != 0
    num = float(max(int(valid.sum()), 1))
    bi = np.broadcast_to(np.arange(B)[:, None], valid.shape)
    pred = head[bi, inds][:, :, list(reg_ch)]                 # (B, K, nc)
    use = valid[:, :, None] & (~np.isnan(tb) if skip_nan else np.ones(tb.shape, bool))
    diff = sub(V(pred), V(np.where(np.isnan(tb) & ~use, 0.0, tb)))
    S = dsum(vabs(diff), use, axis=(0, 1))                    # (nc,)
    cw = f64([fl(c) for c in code_weights[:nc]])
    loc = V(0.0)
    for j in range(nc):
        loc = add(loc, mul(cast32(div(S[j], num, U64)), cw[j], U64), U64)
    loc = mul(loc, loc_weight, U64)
    sg = np.where(use, np.sign(diff.v), 0.0)
    t = div(mul(mul(mul(V(sg), loc_weight), V(cw[None, None, :])), grad_scale), num)
    gv, ge, ga = (np.zeros((B, HW, ld_d)) for _ in range(3))
    cnt = np.zeros((B, HW, ld_d))
    b3 = np.broadcast_to(bi[:, :, None], sg.shape)
    c3 = np.broadcast_to(np.asarray(inds)[:, :, None], sg.shape)
    j3 = np.broadcast_to(np.asarray(reg_ch)[None, None, :], sg.shape)
    nz = sg != 0
    te = np.broadcast_to(t.e, sg.shape)
    if fault == 'last_slot':                                  # a plain store per slot: the last one wins
        for b, k, j in zip(*np.nonzero(nz)):
            gv[b, inds[b, k], reg_ch[j]] = t.v[b, k, j]
    else:
        np.add.at(gv, (b3[nz], c3[nz], j3[nz]), t.v[nz])
    np.add.at(ge, (b3[nz], c3[nz], j3[nz]), te[nz])
    np.add.at(ga, (b3[nz], c3[nz], j3[nz]), np.abs(t.v[nz]) + te[nz])
    np.add.at(cnt, (b3[nz], c3[nz], j3[nz]), 1.0)
    bound = ge + np.maximum(cnt - 1, 0) * U * ga + np.where(cnt > 1, FLUSH, 0.0)
    return loc, gv, bound


HeadDesc = namedtuple('HeadDesc', 'num_class ch_hm reg_ch ld ld_d')


def _one_head(head, heat, tb, inds, mask, hd, cls_weight, loc_weight, code_weights, grad_scale, skip_nan, fault=None):
    B, H, W, ld = head.shape
    assert ld == hd.ld
    hm, npos, g = _focal(head[..., hd.ch_hm:hd.ch_hm + hd.num_class], heat, cls_weight, grad_scale, fault)
    loc, gv, gb = _reg(head.reshape(B, H * W, ld), tb, inds, mask, hd.reg_ch, code_weights, loc_weight, grad_scale, hd.ld_d, skip_nan, fault)
    gv, gb = gv.reshape(B, H, W, hd.ld_d), gb.reshape(B, H, W, hd.ld_d)
    gv[..., hd.ch_hm:hd.ch_hm + hd.num_class] = g.v
    gb[..., hd.ch_hm:hd.ch_hm + hd.num_class] = np.broadcast_to(g.e, g.v.shape)
    tot = cast32(add(hm, loc, U64))
    hm32, loc32 = cast32(hm), cast32(loc)
    losses = np.array([hm32.v, loc32.v, tot.v, float(npos)])
    b_losses = np.array([float(hm32.e), float(loc32.e), float(tot.e), 0.0])
    return losses, b_losses, gv, gb


def centerhead_loss(head, heat, tb, inds, mask, desc, grad_scale, _fault=None):
    """head (B, H, W, ld), heat (B, H, W, ncls), tb (B, K, 8), inds / mask (B, K); desc: dict(num_class, ch_hm, reg_ch, ld_d, cls_weight,
    loc_weight, code_weights).  -> dict: losses [hm, loc, hm + loc, num_pos], dhead (B, H, W, ld_d), b_losses, b_dhead.
    _fault: tests/test_loss_refs_cpu.py's deliberate faults"""
    hd = HeadDesc(desc['num_class'], desc['ch_hm'], tuple(desc['reg_ch']), head.shape[3], desc['ld_d'])
    r = _one_head(head, heat, tb, inds, mask, hd, fl(desc['cls_weight']), fl(desc['loc_weight']), desc['code_weights'], fl(grad_scale),
                  True, _fault)
    return dict(losses=r[0], b_losses=r[1], dhead=r[2], b_dhead=r[3])


def centerhead_loss_ext(heads, desc, grad_scale, _fault=None):
    """heads: list of dict(head, heat, tb, inds, mask, num_class, ch_hm, reg_ch, ld_d); desc: dict(cls_weight, loc_weight, code_weights).
    -> dict: losses (n, 4), b_losses, total, b_total, dheads [..], b_dheads [..]"""
    out = dict(losses=[], b_losses=[], dheads=[], b_dheads=[])
    for h in heads:
        hd = HeadDesc(h['num_class'], h['ch_hm'], tuple(h['reg_ch']), h['head'].shape[3], h['ld_d'])
        assert h['tb'].shape[2] == len(hd.reg_ch)
        r = _one_head(h['head'], h['heat'], h['tb'], h['inds'], h['mask'], hd, fl(desc['cls_weight']), fl(desc['loc_weight']),
                      desc['code_weights'], fl(grad_scale), False, _fault)
        for k, v in zip(('losses', 'b_losses', 'dheads', 'b_dheads'), r):
            out[k].append(v)
    out['losses'], out['b_losses'] = np.array(out['losses']), np.array(out['b_losses'])
    t = V(out['losses'][0, 2], out['b_losses'][0, 2])
    for i in range(1, len(heads)):
        t = add(t, V(out['losses'][i, 2], out['b_losses'][i, 2]))
    out['total'], out['b_total'] = float(t.v), float(t.e)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# AnchorHeadSingle
# ---------------------------------------------------------------------------------------------------------------------

def dir_q(reg6, anchor_rot, dir_offset, dir_period):
    """the bin coordinate off / dir_period of k_anchor_loss in float64, on the float32 constants of the kernel"""
    v = f64(reg6) + f64(anchor_rot) - fl(dir_offset)
    off = v - np.floor(v / TWO_PI32) * TWO_PI32
    return off / fl(dir_period)


def anchor_loss(head, anchors, labels, reg_targets, desc, grad_scale, _fault=None):
    """head (B, H, W, ld), anchors (N, 7), labels (B, N), reg_targets (B, N, 7), N = H W A; desc: dict(anchors_per_loc, num_class,
    num_dir_bins, ld_d, dir_offset, dir_period, cls_weight, loc_weight, dir_weight, code_weights); channels: class, box, direction blocks
    in that order from 0.  -> dict: losses (5,), b_losses, dhead (B, H, W, ld_d), b_dhead, groups: the channel slice of each group"""
    B, H, W, ld = head.shape
    A, nc, nb, ld_d = desc['anchors_per_loc'], desc['num_class'], desc['num_dir_bins'], desc['ld_d']
    N = H * W * A
    ch_box, ch_dir = A * nc, A * nc + A * 7
    used = ch_dir + A * nb
    gs, cls_w, loc_w, dir_w = fl(grad_scale), fl(desc['cls_weight']), fl(desc['loc_weight']), fl(desc['dir_weight'])
    cw = f64([fl(c) for c in desc['code_weights']])
    hp = f64(head).reshape(B, H * W, ld)
    labels = np.asarray(labels)
    pos = labels > 0
    if _fault == 'batch_norm':
        norm = np.full((B, 1), max(float(pos.sum()), 1.0))
    else:
        norm = np.maximum(pos.sum(1, keepdims=True).astype(np.float64), 1.0)
    w1 = div(ONE, V(norm))                                                  # (B, 1)
    inv_b = V(1.0) if _fault == 'no_inv_batch' else div(ONE, float(B))
    # classification
    x = hp[:, :, :ch_box].reshape(B, N, nc)
    w = where(labels >= 0, w1, V(np.zeros((B, 1))))[:, :, None]
    target = np.where(pos, 1 if nc == 1 else labels, 0)
    tt = (target[:, :, None] == np.arange(1, nc + 1)[None, None, :]).astype(np.float64)
    p = sigmoid(x)
    aw = add(mul(V(tt), 0.25), mul(sub(ONE, V(tt)), 0.75))
    pt = add(mul(V(tt), sub(ONE, p)), mul(sub(ONE, V(tt)), p))
    bce = add(sub(V(np.maximum(x, 0.0)), mul(V(x), V(tt))), vlog1p(vexp(V(-np.abs(x)))))
    l_cls = dsum(mul(mul(mul(aw, mul(pt, pt)), bce), w), np.broadcast_to((labels >= 0)[:, :, None], x.shape))
    dpt = mul(mul(sub(ONE, mul(2.0, V(tt))), p), sub(ONE, p))
    g = add(mul(mul(mul(2.0, pt), dpt), bce), mul(mul(pt, pt), sub(p, V(tt))))
    g_cls = mul(mul(mul(mul(mul(aw, g), w), cls_w), inv_b), gs)
    g_cls = where(np.broadcast_to((labels >= 0)[:, :, None], x.shape), g_cls, V(np.zeros_like(x)))
    # localisation
    rw = where(pos, w1, V(np.zeros((B, 1))))[:, :, None]
    pv = hp[:, :, ch_box:ch_dir].reshape(B, N, 7)
    tv = f64(reg_targets)
    use = pos[:, :, None] & ~np.isnan(tv)
    tvz = np.where(np.isnan(tv), 0.0, tv)
    d_lin = sub(V(pv), V(tvz))
    sp, cp, st, ct = vsin(V(pv[..., 6])), vcos(V(pv[..., 6])), vsin(V(tvz[..., 6])), vcos(V(tvz[..., 6]))
    d_rot = sub(mul(sp, ct), mul(cp, st))
    chain6 = add(mul(cp, ct), mul(sp, st))
    is6 = np.arange(7)[None, None, :] == 6
    d = where(is6, V(d_rot.v[..., None], d_rot.e[..., None]), d_lin)
    chain = where(is6, V(chain6.v[..., None], chain6.e[..., None]), V(np.ones_like(pv)))
    d = mul(d, V(cw[None, None, :]))
    a = vabs(d)
    small = a.v < BETA
    near = np.abs(a.v - BETA) <= a.e                          # the kernel may take the other branch: value and slope are continuous
    gap = np.where(near, np.abs(a.v - BETA) + a.e, 0.0)
    sl1 = where(small, div(mul(mul(0.5, a), a), BETA), sub(a, mul(0.5, BETA)))
    sl1 = V(sl1.v, sl1.e + gap * gap / (2 * BETA))
    l_loc = dsum(mul(sl1, rw), use)
    ds = where(small, div(d, BETA), V(np.sign(d.v)))
    ds = V(ds.v, ds.e + gap / BETA)
    g_box = mul(mul(mul(mul(mul(mul(ds, V(cw[None, None, :])), chain), rw), loc_w), inv_b), gs)
    g_box = where(use, g_box, V(np.zeros_like(pv)))
    # direction
    l_dir = V(0.0)
    g_dir = None
    if nb > 0:
        xd = hp[:, :, ch_dir:used].reshape(B, N, nb)
        q = dir_q(np.where(pos, tvz[..., 6], 0.0), f64(anchors)[None, :, 6], desc['dir_offset'], desc['dir_period'])
        bins = np.clip(np.floor(q).astype(np.int64), 0, nb - 1)
        hot = (bins[:, :, None] == np.arange(nb)[None, None, :]).astype(np.float64)
        mx = xd.max(-1, keepdims=True)
        se = fsum(vexp(sub(V(xd), V(mx))), axis=-1, depth=nb - 1)
        lse = add(V(mx[..., 0]), vlog(se))
        xb = (xd * hot).sum(-1)
        l_dir = dsum(mul(sub(lse, V(xb)), rw[:, :, 0]), pos)
        sm = vexp(sub(V(xd), V(lse.v[..., None], lse.e[..., None])))
        g_dir = mul(mul(mul(mul(sub(sm, V(hot)), rw), dir_w), inv_b), gs)
        g_dir = where(np.broadcast_to(pos[:, :, None], xd.shape), g_dir, V(np.zeros_like(xd)))
    # finalize
    Bf = float(B)
    cls = mul(div(l_cls, Bf, U64), cls_w, U64)
    loc = mul(div(l_loc, Bf, U64), loc_w, U64)
    dr = mul(div(l_dir, Bf, U64), dir_w, U64) if nb > 0 else V(0.0)
    tot = cast32(add(add(cls, loc, U64), dr, U64))
    outs = [cast32(cls), cast32(loc), cast32(dr), tot, V(float(pos.sum()))]
    dv, db = np.zeros((B, H * W, ld_d)), np.zeros((B, H * W, ld_d))
    for sl, gg, n in ((slice(0, ch_box), g_cls, nc), (slice(ch_box, ch_dir), g_box, 7), (slice(ch_dir, used), g_dir, nb)):
        if gg is not None:
            dv[:, :, sl] = gg.v.reshape(B, H * W, A * n)
            db[:, :, sl] = np.broadcast_to(gg.e, gg.v.shape).reshape(B, H * W, A * n)
    return dict(losses=np.array([float(o.v) for o in outs]), b_losses=np.array([float(o.e) for o in outs]),
                dhead=dv.reshape(B, H, W, ld_d), b_dhead=db.reshape(B, H, W, ld_d),
                groups=dict(cls=slice(0, ch_box), box=slice(ch_box, ch_dir), dir=slice(ch_dir, used), pad=slice(used, ld_d)))


# ---------------------------------------------------------------------------------------------------------------------
# distillation
# ---------------------------------------------------------------------------------------------------------------------

def _softmax(x):
    m = x.max(-1, keepdims=True)
    E = vexp(sub(V(x), V(m)))
    s = fsum(E, axis=-1, depth=DIST_DEPTH)
    return div(E, V(s.v[..., None], s.e[..., None]))


def distill_loss(fused, early, c, weight, grad_scale, accumulate=False, prior=None, _fault=None):
    """fused, early (pixels, >= c): the first c columns are read.  -> dict: loss, b_loss, dfused (pixels, c), b_dfused"""
    f, e = f64(fused)[:, :c], f64(early)[:, :c]
    pixels = f.shape[0]
    wt, gs = fl(weight), fl(grad_scale)
    a, b = _softmax(f), _softmax(e)
    d = sub(a, b)
    assert (np.abs(d.v) + d.e < 1.0).all()
    n = float(pixels) * float(c)
    S = dsum(mul(mul(0.5, d), d))
    loss = cast32(mul(div(S, float(pixels) if _fault == 'mean_pixels' else n, U64), wt, U64))
    dot = fsum(mul(d, a), axis=-1, depth=DIST_DEPTH)
    if _fault == 'no_dot':
        dot = V(np.zeros(pixels))
    k = mul(mul(wt, gs), cast32(div(ONE, n, U64)))
    g = mul(mul(k, a), sub(d, V(dot.v[..., None], dot.e[..., None])))
    if accumulate:
        g = add(V(f64(prior)[:, :c]), g)
    return dict(loss=float(loss.v), b_loss=float(loss.e), dfused=g.v, b_dfused=np.broadcast_to(g.e, g.v.shape))


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every case names the code path it is there for
# ---------------------------------------------------------------------------------------------------------------------

PLANT = 1.25 * CLAMP_MARGIN       # where the generators put a logit next to a threshold: the margin plus room for the float32 rounding
PLANTED_LOGITS = [X_LO - PLANT, X_LO + PLANT, X_HI - PLANT, X_HI + PLANT, 12.0, -12.0, 30.0, -30.0, X_LO - 2 * PLANT, X_HI + 2 * PLANT]


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _logits(rng, shape, lo=-6.0, hi=6.0, every=7):
    """uniform logits with the planted ones (both sides of both clamp thresholds at the margin, far inside and far outside) at every
    `every`-th element; anything a draw put closer to a threshold than the margin is moved out to it"""
    x = rng.uniform(lo, hi, size=shape).astype(F32)
    flat = x.reshape(-1)
    idx = np.arange(0, flat.size, every)
    flat[idx] = np.array(PLANTED_LOGITS, F32)[np.arange(idx.size) % len(PLANTED_LOGITS)]
    for thr in (X_LO, X_HI):
        close = np.abs(f64(flat) - thr) < CLAMP_MARGIN
        flat[close] = (thr + np.where(f64(flat[close]) >= thr, PLANT, -PLANT)).astype(F32)
    return x


def _plant_targets(rng, head2, inds, mask, reg_ch, equal_every=11):
    """targets = the head value at the slot's cell + a difference of magnitude in [2^-9, 2] and random sign; every equal_every-th (slot,
    code) holds the head value itself (difference exactly 0)"""
    B, K = inds.shape
    bi = np.broadcast_to(np.arange(B)[:, None], (B, K))
    pred = head2[bi, inds][:, :, list(reg_ch)]
    mag = rng.uniform(2.0 ** -9, 2.0, size=pred.shape)
    sgn = np.where(rng.random(pred.shape) < 0.5, -1.0, 1.0)
    tb = (f64(pred) + sgn * mag).astype(F32)
    eq = (np.arange(pred.size).reshape(pred.shape) % equal_every) == 3
    tb[eq] = pred[eq]
    return tb, pred


CH = namedtuple('CH', 'B H W ncls K ld ld_d ch_hm grad_scale flavour why')

CH_CASES = [
    CH(3, 7, 9, 1, 8, 16, 16, 8, 1.0, 'mixed', 'frame 1 without a valid slot; 2 and 3 slots per cell, opposing and equal signs; a NaN column'),
    CH(2, 5, 5, 3, 500, 16, 24, 0, 0.37, 'mixed', 'K = 500 on 25 cells: up to dozens of atomics per cell; ld_d > ld; grad_scale 0.37'),
    CH(1, 1, 1, 1, 1, 9, 9, 3, 0.37, 'mixed', 'one cell, one slot, every channel of the row used'),
    CH(2, 40, 52, 5, 32, 16, 16, 11, 1.0, 'mixed', '20800 heat-map elements: 82 blocks of k_focal_reduce'),
    CH(1, 1, 1, 1, 1, 9, 9, 3, 1.0, 'empty', 'no valid slot and no peak in the whole batch: num_pos == 0, num -> 1'),
    CH(2, 5, 5, 3, 500, 16, 24, 0, 0.37, 'empty', 'the same on a batch of two'),
    CH(1, 182, 181, 8, 4, 16, 16, 8, 1.0, 'mixed', '263536 heat-map elements > 1024 blocks * 256: a second trip of the grid-stride loop '
       '(the 20800 of case 3 stay inside one sweep: the block cap is 1024, not 64)'),
]
CODE_WEIGHTS = [1.0, 1.0, 0.5, 1.0, 2.0, 1.0, 0.25, 1.5, 0.2, 0.2, 1.25, 1.0, 1.0, 1.0, 1.0, 1.0]


def _heat_and_slots(rng, B, H, W, ncls, K, valid_frac, empty_frames=(), shared=True):
    """a heat map below 1 with a peak of exactly 1 at the cell of every valid slot, cells drawn so that several slots share one"""
    heat = (rng.uniform(0.0, 0.95, size=(B, H, W, ncls)) ** 3).astype(F32)
    heat[rng.random(heat.shape) < 0.3] = 0.0
    inds = rng.integers(0, H * W, size=(B, K)).astype(np.int32)
    mask = (rng.random((B, K)) < valid_frac).astype(np.int32)
    if shared and K >= 5:
        for b in range(B):
            inds[b, 1] = inds[b, 0]                           # two slots on one cell
            inds[b, 3] = inds[b, 4] = inds[b, 2]              # three slots on one cell
            mask[b, :5] = 1
    for b in empty_frames:
        mask[b] = 0
    cls = rng.integers(0, ncls, size=(B, K))
    for b, k in zip(*np.nonzero(mask)):
        heat[b, inds[b, k] // W, inds[b, k] % W, cls[b, k]] = 1.0
    return heat, inds, mask


def _shared_signs(tb, pred, reg_ch):
    """slots 0, 1 (one cell): opposing signs on code 0, equal on code 1; slots 2, 3, 4 (one cell): +, +, + on code 0 and +, -, + on code 1"""
    for k, s0, s1 in ((0, 1, 1), (1, -1, 1), (2, 1, 1), (3, 1, -1), (4, 1, 1)):
        tb[:, k, 0] = (f64(pred[:, k, 0]) - s0 * 0.375).astype(F32)
        tb[:, k, 1] = (f64(pred[:, k, 1]) - s1 * 0.625).astype(F32)


@functools.lru_cache(maxsize=None)
def ch_data(i):
    """inputs of CH_CASES[i] (float32 / int32), its descriptor dict and the reference; read-only"""
    c = CH_CASES[i]
    rng = np.random.default_rng(7000 + i)
    head = rng.uniform(-3.0, 3.0, size=(c.B, c.H, c.W, c.ld)).astype(F32)
    head[..., c.ch_hm:c.ch_hm + c.ncls] = _logits(rng, (c.B, c.H, c.W, c.ncls))
    others = [ch for ch in range(c.ld) if not c.ch_hm <= ch < c.ch_hm + c.ncls]
    reg_ch = [int(v) for v in rng.permutation(others)[:8]]
    empty = c.flavour == 'empty'
    heat, inds, mask = _heat_and_slots(rng, c.B, c.H, c.W, c.ncls, c.K, 0.0 if empty else 0.6,
                                       empty_frames=(1,) if (c.B == 3 and not empty) else (), shared=not empty)
    if c.K == 1 and not empty:
        mask[:] = 1
        heat[0, 0, 0, 0] = 1.0
    tb, pred = _plant_targets(rng, head.reshape(c.B, c.H * c.W, c.ld), inds, mask, reg_ch)
    if c.K >= 5:
        _shared_signs(tb, pred, reg_ch)
    if i == 0:
        tb[:, :, 5] = np.nan
    desc = dict(num_class=c.ncls, ch_hm=c.ch_hm, reg_ch=reg_ch, ld_d=c.ld_d, cls_weight=1.0, loc_weight=0.25, code_weights=CODE_WEIGHTS[:8])
    d = dict(head=head, heat=heat, tb=tb, inds=inds, mask=mask, desc=desc, grad_scale=c.grad_scale)
    d['ref'] = _frozen(centerhead_loss(head, heat, tb, inds, mask, desc, c.grad_scale))
    return _frozen(d)


EXT = namedtuple('EXT', 'B H W K heads grad_scale why')          # heads: (num_class, n_codes, ld, ld_d, with positives)

EXT_CASES = [
    EXT(2, 5, 7, 6, ((1, 8, 12, 9, True),), 1.0, 'one head, ld_d < ld'),
    EXT(2, 40, 52, 8, ((2, 10, 16, 13, False), (4, 11, 18, 20, True)), 0.37,
        'head 1: 16640 heat-map elements > 64 * 256, the second trip of k_lossx_reduce; head 0 without positives beside it'),
    EXT(3, 6, 5, 100, tuple((n, k, 19 + (j % 3), 16 + (j % 2), j != 5) for j, (n, k) in
                            enumerate(((1, 8), (2, 10), (4, 11), (1, 11), (2, 8), (4, 10), (1, 10), (2, 11)))), 0.5,
        'PCP_DET_MAX_HEADS heads; B K = 300 > 256 with frame 2 slots 50..60 on one cell, across the 256-thread boundary; head 5 empty'),
]


@functools.lru_cache(maxsize=None)
def ext_data(i):
    c = EXT_CASES[i]
    rng = np.random.default_rng(7100 + i)
    heads = []
    for hi, (ncls, ncodes, ld, ld_d, has_pos) in enumerate(c.heads):
        lim = min(ld, ld_d)
        ch_hm = int(rng.integers(0, lim - ncls - ncodes + 1)) if hi % 2 == 0 else (lim - ncls - ncodes) // 2      # never required to be last
        head = rng.uniform(-3.0, 3.0, size=(c.B, c.H, c.W, ld)).astype(F32)
        head[..., ch_hm:ch_hm + ncls] = _logits(rng, (c.B, c.H, c.W, ncls))
        others = [ch for ch in range(lim) if not ch_hm <= ch < ch_hm + ncls]
        reg_ch = [int(v) for v in rng.permutation(others)[:ncodes]]
        heat, inds, mask = _heat_and_slots(rng, c.B, c.H, c.W, ncls, c.K, 0.7 if has_pos else 0.0, shared=has_pos)
        if has_pos and c.K >= 61:
            inds[2, 50:61] = inds[2, 50]
            mask[2, 50:61] = 1
            for k in range(50, 61):
                heat[2, inds[2, k] // c.W, inds[2, k] % c.W, 0] = 1.0
        tb, pred = _plant_targets(rng, head.reshape(c.B, c.H * c.W, ld), inds, mask, reg_ch)
        if has_pos:
            _shared_signs(tb, pred, reg_ch)
        heads.append(dict(head=head, heat=heat, tb=tb, inds=inds, mask=mask, num_class=ncls, ch_hm=ch_hm, reg_ch=reg_ch, ld_d=ld_d))
    desc = dict(cls_weight=1.0, loc_weight=0.25, code_weights=CODE_WEIGHTS)
    d = dict(heads=heads, desc=desc, grad_scale=c.grad_scale)
    d['ref'] = centerhead_loss_ext(heads, desc, c.grad_scale)
    for h in heads:
        _frozen(h)
    return d


AN = namedtuple('AN', 'B H W A ncls bins ld ld_d grad_scale why')

AN_CASES = [
    AN(2, 5, 7, 2, 1, 2, 20, 23, 0.5, 'class-agnostic target; ld = used; frame 1 without positives beside frame 0 with many'),
    AN(3, 6, 11, 6, 3, 2, 75, 72, 0.5, 'ld = used + 3, ld_d = used; 396 anchors per frame: two blocks of k_anchor_loss'),
    AN(1, 9, 9, 2, 16, 0, 80, 49, 1.0, 'AL_MAX_CLASS classes, no direction classifier, ld = 80'),
    AN(2, 4, 4, 6, 3, 8, 111, 108, 0.5, 'AL_MAX_BINS direction bins'),
]
AN_WEIGHTS = dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0, 1.0, 1.0, 0.5, 1.0, 2.0, 1.0])
DIR_OFFSET = 0.78539


@functools.lru_cache(maxsize=None)
def an_data(i):
    c = AN_CASES[i]
    rng = np.random.default_rng(7200 + i)
    N = c.H * c.W * c.A
    used = c.A * (c.ncls + 7 + c.bins)
    ch_box, ch_dir = c.A * c.ncls, c.A * c.ncls + c.A * 7
    head = np.full((c.B, c.H, c.W, c.ld), 1e30, F32)         # the padding channels of the head are never read
    head[..., :ch_box] = _logits(rng, (c.B, c.H, c.W, ch_box), -5.0, 5.0)
    head[..., ch_box:ch_dir] = rng.uniform(-1.5, 1.5, size=(c.B, c.H, c.W, c.A * 7)).astype(F32)
    head[..., ch_dir:used] = rng.uniform(-3.0, 3.0, size=(c.B, c.H, c.W, c.A * c.bins)).astype(F32)
    anchors = rng.uniform(-1.0, 1.0, size=(N, 7)).astype(F32)
    anchors[:, 6] = np.where(np.arange(N) % 2 == 0, 0.0, np.pi / 2).astype(F32)
    r = rng.random((c.B, N))
    labels = np.where(r < 0.15, -1, np.where(r < 0.6, 0, rng.integers(1, c.ncls + 1, size=(c.B, N)))).astype(np.int32)
    if c.B > 1:
        labels[1][labels[1] > 0] = 0                          # a frame without positives: its normaliser clamps at 1
    box = head[..., ch_box:ch_dir].reshape(c.B, N, 7)
    mag = rng.uniform(2.0 ** -9, 1.0, size=box.shape)
    mag[rng.random(box.shape) < 0.4] *= 0.05                  # both smooth-L1 branches (beta = 1/9)
    reg = (f64(box) + np.where(rng.random(box.shape) < 0.5, -1.0, 1.0) * mag).astype(F32)
    eq = (np.arange(reg.size).reshape(reg.shape) % 13) == 5
    reg[eq] = box[eq]
    if c.bins > 0:                                            # headings by their bin coordinate: 0.1 .. 0.9 into a bin, wraps -1, 0, +1
        period = fl(2 * np.pi / c.bins)
        q = rng.integers(0, c.bins, size=(c.B, N)) + rng.uniform(0.1, 0.9, size=(c.B, N))
        wrap = rng.integers(-1, 2, size=(c.B, N))
        reg[..., 6] = (q * period + wrap * TWO_PI32 + fl(DIR_OFFSET) - f64(anchors)[None, :, 6]).astype(F32)
    nanpos = (rng.random(reg.shape) < 0.05) & (np.arange(7)[None, None, :] < 6)
    reg[nanpos] = np.nan
    desc = dict(anchors_per_loc=c.A, num_class=c.ncls, num_dir_bins=c.bins, ld_d=c.ld_d, dir_offset=DIR_OFFSET,
                dir_period=2 * np.pi / c.bins if c.bins else 0.0, **AN_WEIGHTS)
    d = dict(head=head, anchors=anchors, labels=labels, reg=reg, desc=desc, grad_scale=c.grad_scale)
    d['ref'] = _frozen(anchor_loss(head, anchors, labels, reg, desc, c.grad_scale))
    return _frozen(d)


DIST_MAX_C = 512                 # 64 * DIST_MAXV of k_distill
DS = namedtuple('DS', 'c pixels weight grad_scale accumulate')
DS_CASES = [DS(c, px, (10.0, 0.25)[(i + j) % 2], (1.0, 0.37)[j % 2], (i + j) % 3 == 0)
            for i, c in enumerate((1, 63, 64, 65, 100, 384, 512)) for j, px in enumerate((1, 3, 257))]
ROW_KINDS = ('spread', 'equal', 'plain')          # logit spread of +-40 | fused == early | +-3


def ds_row_kinds(case):
    """the kind of every row: rows 0, 5, 10, .. spread, rows 1, 6, 11, .. equal; a single row takes its kind from c"""
    if case.pixels == 1:
        return [ROW_KINDS[case.c % 3]]
    return [ROW_KINDS[min(p % 5, 2)] for p in range(case.pixels)]


@functools.lru_cache(maxsize=None)
def ds_data(i):
    """fused (pixels, c + 3), early (pixels, c + 5), prior (pixels, c + 2): 1e30 beyond c in the inputs"""
    c = DS_CASES[i]
    rng = np.random.default_rng(7300 + i)
    fused = np.full((c.pixels, c.c + 3), 1e30, F32)
    early = np.full((c.pixels, c.c + 5), 1e30, F32)
    fused[:, :c.c] = rng.uniform(-3.0, 3.0, size=(c.pixels, c.c)).astype(F32)
    early[:, :c.c] = rng.uniform(-3.0, 3.0, size=(c.pixels, c.c)).astype(F32)
    for p, kind in enumerate(ds_row_kinds(c)):
        if kind == 'spread':
            fused[p, :c.c] = rng.uniform(-40.0, 40.0, size=c.c).astype(F32)
            early[p, :c.c] = rng.uniform(-40.0, 40.0, size=c.c).astype(F32)
            fused[p, 0], fused[p, c.c - 1], early[p, c.c // 2] = 40.0, -40.0, 40.0
        elif kind == 'equal':
            early[p, :c.c] = fused[p, :c.c]
    prior = rng.uniform(-1e-3, 1e-3, size=(c.pixels, c.c + 2)).astype(F32)
    d = dict(fused=fused, early=early, prior=prior)
    d['ref'] = _frozen(distill_loss(fused, early, c.c, c.weight, c.grad_scale, c.accumulate, prior))
    return _frozen(d)
