"""The float64 references, bounds and case tables of tests/loss_refs.py, checked on the CPU: the references against torch float64 autograd
of the oracle's loss functions (oracle/train.py, oracle/anchor.py) on every case the GPU tests run, the margins that keep every input away
from a discontinuity of the kernels, and eight deliberate faults, each of which has to leave a bound on a named case.  No GPU."""
import numpy as np
import pytest
import torch

import loss_refs as lr
from oracle import anchor as oan
from oracle import train as otr


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _close(got, want, what, rtol=1e-9):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert np.shape(got) == want.shape, (what, np.shape(got), want.shape)
    assert np.allclose(got, want, rtol=rtol, atol=1e-18), (what, float(np.abs(got - want).max()))


# ---- the references against torch float64 autograd --------------------------------------------------------------------------------------

def _torch_head(h, num_class, ch_hm, reg_ch, cls_w, loc_w, code_weights, grad_scale):
    """-> ([hm, loc, hm + loc, num_pos], dL/dhead * grad_scale (B, H, W, ld)) by autograd on the oracle's focal and regression losses"""
    x = _t(h['head']).requires_grad_(True)
    B, H, W, ld = x.shape
    heat, tb = _t(h['heat']), _t(h['tb'])
    inds, mask = torch.from_numpy(np.array(h['inds'], dtype=np.int64)), torch.from_numpy(np.array(h['mask'], dtype=np.int64))
    hm = torch.clamp(x[..., ch_hm:ch_hm + num_class].sigmoid(), min=lr.LO, max=lr.HI)
    hm_loss = otr.focal_loss(hm, heat) * lr.fl(cls_w)
    cw = _t([lr.fl(c) for c in code_weights[:len(reg_ch)]])
    if torch.isnan(tb).any():                     # the oracle multiplies NaN by a zero mask: the kernel's rule (skip the element) in four lines
        pred = x.reshape(B, H * W, ld)[torch.arange(B)[:, None], inds][:, :, list(reg_ch)]
        m = mask[:, :, None].double() * (~torch.isnan(tb)).double()
        rl = ((pred - torch.nan_to_num(tb)).abs() * m).sum(dim=(0, 1)) / torch.clamp_min(mask.double().sum(), 1.0)
    else:
        rl = otr.reg_loss(x.permute(0, 3, 1, 2)[:, list(reg_ch)], mask, inds, tb)
    loc_loss = (rl * cw).sum() * lr.fl(loc_w)
    ((hm_loss + loc_loss) * lr.fl(grad_scale)).backward()
    npos = float((heat == 1).sum())
    return [float(hm_loss.detach()), float(loc_loss.detach()), float((hm_loss + loc_loss).detach()), npos], x.grad.numpy()


def _check_head(ref_losses, ref_dhead, want_losses, want_grad, what):
    _close(ref_losses, np.array(want_losses), what + ' losses')
    n = min(ref_dhead.shape[3], want_grad.shape[3])
    _close(ref_dhead[..., :n], want_grad[..., :n], what + ' dhead')
    assert not ref_dhead[..., n:].any() and not want_grad[..., n:].any()


@pytest.mark.parametrize('i', range(len(lr.CH_CASES)))
def test_centerhead_reference_equals_float64_autograd(i):
    d = lr.ch_data(i)
    ds = d['desc']
    want = _torch_head(d, ds['num_class'], ds['ch_hm'], ds['reg_ch'], ds['cls_weight'], ds['loc_weight'], ds['code_weights'], d['grad_scale'])
    _check_head(d['ref']['losses'], d['ref']['dhead'], *want, 'case %d' % i)
    assert (d['ref']['b_dhead'] >= 0).all() and (d['ref']['b_losses'] >= 0).all()


@pytest.mark.parametrize('i', range(len(lr.EXT_CASES)))
def test_centerhead_ext_reference_equals_float64_autograd(i):
    d = lr.ext_data(i)
    ds, ref = d['desc'], d['ref']
    tot = 0.0
    for hi, h in enumerate(d['heads']):
        want = _torch_head(h, h['num_class'], h['ch_hm'], h['reg_ch'], ds['cls_weight'], ds['loc_weight'], ds['code_weights'], d['grad_scale'])
        _check_head(ref['losses'][hi], ref['dheads'][hi], *want, 'case %d head %d' % (i, hi))
        tot += want[0][2]
    assert abs(ref['total'] - tot) <= 1e-12 * abs(tot) and ref['b_total'] > 0


@pytest.mark.parametrize('i', range(len(lr.AN_CASES)))
def test_anchor_reference_equals_float64_autograd(i):
    c, d = lr.AN_CASES[i], lr.an_data(i)
    ds, ref = d['desc'], d['ref']
    used = c.A * (c.ncls + 7 + c.bins)
    x = _t(d['head'][..., :used]).requires_grad_(True)
    ch_box, ch_dir = c.A * c.ncls, c.A * (c.ncls + 7)
    cfg = dict(LOSS_CONFIG=dict(LOSS_WEIGHTS={k: (lr.fl(v) if k != 'code_weights' else v) for k, v in lr.AN_WEIGHTS.items()}),
               NUM_DIR_BINS=c.bins, DIR_OFFSET=lr.fl(lr.DIR_OFFSET))
    labels = torch.from_numpy(np.array(d['labels'], dtype=np.int64))
    total, terms = oan.losses(x[..., :ch_box].contiguous(), x[..., ch_box:ch_dir].contiguous(),
                              x[..., ch_dir:used].contiguous() if c.bins else None, _t(d['anchors']), labels, _t(d['reg']), cfg, c.ncls)
    (total * lr.fl(d['grad_scale'])).backward()
    want = [float(terms['rpn_loss_cls'].detach()), float(terms['rpn_loss_loc'].detach()),
            float(terms['rpn_loss_dir'].detach()) if c.bins else 0.0, float(total.detach()),
            float((labels > 0).sum())]
    # the oracle's beta is the double 1 / 9, the kernel's and the reference's the float32 one, 3e-8 away: the smooth-L1 terms follow it
    grp = ref['groups']
    _close(ref['losses'][[0, 2, 4]], np.array(want)[[0, 2, 4]], 'losses')
    _close(ref['losses'][[1, 3]], np.array(want)[[1, 3]], 'loc loss', rtol=2.0 ** -23)
    for g in ('cls', 'dir'):
        _close(ref['dhead'][..., grp[g]], x.grad[..., grp[g]], g)
    _close(ref['dhead'][..., grp['box']], x.grad[..., grp['box']], 'box', rtol=2.0 ** -23)
    assert not ref['dhead'][..., used:].any() and ref['dhead'].shape[3] == c.ld_d
    for g in ('cls', 'box', 'dir'):
        if g != 'dir' or c.bins:
            assert np.abs(ref['dhead'][..., ref['groups'][g]]).max() > 0
    # what the table promises about its labels and targets
    lab = d['labels']
    assert (lab == -1).any() and (lab == 0).any() and (lab > 0).any()
    assert np.isnan(d['reg'][lab > 0]).any() and not np.isnan(d['reg'][..., 6]).any()
    if c.B > 1:
        per_frame = (lab > 0).sum(1)
        assert per_frame[1] == 0 and per_frame[0] > 10


@pytest.mark.parametrize('i', range(len(lr.DS_CASES)))
def test_distill_reference_equals_float64_autograd(i):
    c, d = lr.DS_CASES[i], lr.ds_data(i)
    f = _t(d['fused'][:, :c.c]).requires_grad_(True)
    loss = otr.distill_loss(f, _t(d['early'][:, :c.c])) / 10.0 * lr.fl(c.weight)
    (loss * lr.fl(c.grad_scale)).backward()
    ref = d['ref']
    assert abs(ref['loss'] - float(loss.detach())) <= 1e-9 * abs(float(loss.detach())) + 1e-300
    want = f.grad.numpy() + (np.array(d['prior'][:, :c.c], dtype=np.float64) if c.accumulate else 0.0)
    assert np.allclose(ref['dfused'], want, rtol=1e-9, atol=1e-15 * np.abs(want).max() + 1e-300)
    assert (ref['b_dfused'] > 0).all() and ref['b_loss'] > 0


# ---- the margins: no compared element sits at a discontinuity -----------------------------------------------------------------------------

def _heat_logits():
    for i in range(len(lr.CH_CASES)):
        d = lr.ch_data(i)
        yield 'ch %d' % i, d['head'][..., d['desc']['ch_hm']:d['desc']['ch_hm'] + d['desc']['num_class']]
    for i in range(len(lr.EXT_CASES)):
        for hi, h in enumerate(lr.ext_data(i)['heads']):
            yield 'ext %d head %d' % (i, hi), h['head'][..., h['ch_hm']:h['ch_hm'] + h['num_class']]


def test_heat_map_logits_keep_the_margin_from_both_clamp_thresholds():
    seen = set()
    for what, x in _heat_logits():
        x = lr.f64(x).reshape(-1)
        for thr in (lr.X_LO, lr.X_HI):
            assert np.abs(x - thr).min() >= lr.CLAMP_MARGIN, what
        _p, inside, s = lr.clamped_sigmoid(x)
        # the margin in s, against what the three roundings of s can move it: at least 8 times, so `inside` is the kernel's
        assert (np.minimum(np.abs(s.v - lr.LO), np.abs(s.v - lr.HI)) >= 8 * s.e).all(), what
        if x.size >= 70:
            for name, thr, side in (('lo-', lr.X_LO, -1), ('lo+', lr.X_LO, 1), ('hi-', lr.X_HI, -1), ('hi+', lr.X_HI, 1)):
                near = (side * (x - thr) > 0) & (np.abs(x - thr) < 1.5 * lr.CLAMP_MARGIN)
                assert near.any(), (what, name)
                assert bool(inside[near].all()) == (name in ('lo+', 'hi-')) and bool((~inside[near]).all()) == (name in ('lo-', 'hi+'))
            for far in (12.0, -12.0, 30.0, -30.0):
                assert (x == far).any(), (what, far)
            seen.add(what)
    assert len(seen) >= 5 + sum(len(c.heads) for c in lr.EXT_CASES)       # every case but the two of one cell


def _l1_sets():
    for i in range(len(lr.CH_CASES)):
        d = lr.ch_data(i)
        yield 'ch %d' % i, d['head'], d['tb'], d['inds'], d['mask'], d['desc']['reg_ch']
    for i in range(len(lr.EXT_CASES)):
        for hi, h in enumerate(lr.ext_data(i)['heads']):
            yield 'ext %d head %d' % (i, hi), h['head'], h['tb'], h['inds'], h['mask'], h['reg_ch']


def test_l1_differences_are_exactly_zero_or_at_least_the_margin():
    zeros = large = 0
    for what, head, tb, inds, mask, reg_ch in _l1_sets():
        B, H, W, ld = head.shape
        pred = lr.f64(head).reshape(B, H * W, ld)[np.arange(B)[:, None], inds][:, :, list(reg_ch)]
        use = (mask != 0)[:, :, None] & ~np.isnan(tb)
        diff = np.abs(pred - lr.f64(tb))[use]
        assert ((diff == 0) | (diff >= lr.L1_MARGIN)).all(), what
        zeros, large = zeros + int((diff == 0).sum()), large + int((diff > 0).sum())
        if what.startswith('ext'):
            assert not np.isnan(tb).any(), what                # finite by the contract of the ext entry point
    assert zeros > 50 and large > 1000
    assert np.isnan(lr.ch_data(0)['tb'][:, :, 5]).all()


def test_shared_cells_hold_two_and_three_slots_with_opposing_and_equal_signs():
    for d, heads in [(lr.ch_data(0), None), (lr.ch_data(1), None)] + [(None, lr.ext_data(i)['heads']) for i in range(len(lr.EXT_CASES))]:
        for h in ([d] if heads is None else heads):
            if not h['mask'].any():
                continue
            inds, mask, tb = h['inds'], h['mask'], h['tb']
            reg_ch = h['desc']['reg_ch'] if heads is None else h['reg_ch']
            B, H, W, ld = h['head'].shape
            b = 0
            assert inds[b, 0] == inds[b, 1] and inds[b, 2] == inds[b, 3] == inds[b, 4] and mask[b, :5].all()
            pred = lr.f64(h['head']).reshape(B, H * W, ld)[b, inds[b, :5]][:, list(reg_ch)]
            sg = np.sign(pred - lr.f64(tb[b, :5]))
            assert sg[0, 0] == -sg[1, 0] != 0 and sg[0, 1] == sg[1, 1] != 0
            assert sg[2, 0] == sg[3, 0] == sg[4, 0] != 0 and sg[2, 1] == -sg[3, 1] == sg[4, 1] != 0
    e2 = lr.ext_data(2)['heads'][0]
    k = lr.EXT_CASES[2].K
    assert (e2['inds'][2, 50:61] == e2['inds'][2, 50]).all() and e2['mask'][2, 50:61].all() and 2 * k + 50 < 256 < 2 * k + 61


def test_table_shapes_reach_the_loops_they_are_there_for():
    c = lr.CH_CASES[-1]
    assert c.B * c.H * c.W * c.ncls > lr.FOCAL_SWEEP
    e = lr.EXT_CASES[1]
    assert e.B * e.H * e.W * e.heads[1][0] > lr.LX_STRIDE and not lr.ext_data(1)['heads'][0]['mask'].any()
    assert len(lr.EXT_CASES[2].heads) == lr.MAX_HEADS and lr.EXT_CASES[2].B * lr.EXT_CASES[2].K > 256
    assert {h[1] for c in lr.EXT_CASES for h in c.heads} == {8, 10, 11} and {h[0] for c in lr.EXT_CASES for h in c.heads} == {1, 2, 4}
    assert all(h[2] != h[3] for c in lr.EXT_CASES for h in c.heads)
    for i in range(len(lr.EXT_CASES)):
        for h in lr.ext_data(i)['heads']:
            assert sorted(h['reg_ch']) != list(h['reg_ch'])          # shuffled
    assert any(h['ch_hm'] + h['num_class'] < min(h['head'].shape[3], h['ld_d']) for i in range(len(lr.EXT_CASES)) for h in lr.ext_data(i)['heads'])
    assert lr.ch_data(4)['ref']['losses'][3] == 0 and lr.ch_data(5)['ref']['losses'][3] == 0 and not lr.ch_data(5)['mask'].any()
    assert not lr.ch_data(0)['mask'][1].any() and lr.ch_data(0)['mask'][0].any()
    assert {k for c in lr.DS_CASES for k in lr.ds_row_kinds(c)} == set(lr.ROW_KINDS)
    assert {(c.c, c.pixels) for c in lr.DS_CASES} == {(c, p) for c in (1, 63, 64, 65, 100, 384, 512) for p in (1, 3, 257)}


def test_headings_keep_the_margin_from_every_direction_bin_edge():
    below = above = 0
    for i, c in enumerate(lr.AN_CASES):
        if not c.bins:
            continue
        d = lr.an_data(i)
        pos = d['labels'] > 0
        q = lr.dir_q(d['reg'][..., 6], d['anchors'][None, :, 6], d['desc']['dir_offset'], d['desc']['dir_period'])[pos]
        assert (np.abs(q - np.round(q)) >= lr.DIR_MARGIN).all() and q.min() > 0 and q.max() < c.bins
        assert set(np.floor(q).astype(int)) == set(range(c.bins))
        v = (lr.f64(d['reg'][..., 6]) + lr.f64(d['anchors'])[None, :, 6] - lr.fl(lr.DIR_OFFSET))[pos]
        below, above = below + int((v < 0).sum()), above + int((v >= lr.TWO_PI32).sum())
    assert below > 10 and above > 10


# ---- teeth: eight deliberate faults, each caught by a named case -----------------------------------------------------------------------------

def _worst_head(ref, bad):
    return max(lr.worst(bad['losses'], ref['losses'], ref['b_losses']), lr.worst(bad['dhead'], ref['dhead'], ref['b_dhead']))


def _ch_fault(i, fault):
    d = lr.ch_data(i)
    bad = lr.centerhead_loss(d['head'], d['heat'], d['tb'], d['inds'], d['mask'], d['desc'], d['grad_scale'], _fault=fault)
    return _worst_head(d['ref'], bad)


def _ext_fault(i, fault):
    d = lr.ext_data(i)
    ref, bad = d['ref'], lr.centerhead_loss_ext(d['heads'], d['desc'], d['grad_scale'], _fault=fault)
    return max(lr.worst(bad['dheads'][h], ref['dheads'][h], ref['b_dheads'][h]) for h in range(len(d['heads'])))


def _an_fault(i, fault):
    d = lr.an_data(i)
    ref, bad = d['ref'], lr.anchor_loss(d['head'], d['anchors'], d['labels'], d['reg'], d['desc'], d['grad_scale'], _fault=fault)
    return _worst_head(ref, bad)


def _ds_fault(i, fault):
    c, d = lr.DS_CASES[i], lr.ds_data(i)
    ref, bad = d['ref'], lr.distill_loss(d['fused'], d['early'], c.c, c.weight, c.grad_scale, c.accumulate, d['prior'], _fault=fault)
    return max(lr.worst(bad['dfused'], ref['dfused'], ref['b_dfused']),
               lr.worst(np.array(bad['loss']), np.array(ref['loss']), np.array(ref['b_loss'])))


FAULTS = [      # (fault, table, the case that catches it)
    ('neg_exp2', _ch_fault, 0),           # negative weight (1 - gt)^2 in the place of (1 - gt)^4
    ('no_clamp_zero', _ch_fault, 0),      # a gradient outside the clamp
    ('last_slot', _ch_fault, 0),          # a store per slot: the last slot of a shared cell wins (atomics path)
    ('last_slot', _ext_fault, 0),         # the same on the slot-order path
    ('fp32_sum', _ch_fault, 6),           # one fp32 accumulator over 263536 focal terms
    ('batch_norm', _an_fault, 0),         # positives of the batch in the place of the frame's
    ('no_inv_batch', _an_fault, 0),       # gradient without 1 / batch
    ('no_dot', _ds_fault, 4),             # softmax Jacobian without the - dot term
    ('mean_pixels', _ds_fault, 4),        # mean over the pixels only
]


@pytest.mark.parametrize('fault,table,case', FAULTS, ids=['%s-%s-%d' % (f, t.__name__.strip('_'), c) for f, t, c in FAULTS])
def test_every_deliberate_fault_leaves_the_bound_on_its_named_case(fault, table, case):
    r = table(case, fault)
    assert r > 1.0, '%s passes case %d: ratio %r' % (fault, case, r)


def test_the_faultless_reference_is_its_own_fixed_point():
    d = lr.ch_data(2)
    again = lr.centerhead_loss(d['head'], d['heat'], d['tb'], d['inds'], d['mask'], d['desc'], d['grad_scale'])
    assert _worst_head(d['ref'], again) == 0.0
