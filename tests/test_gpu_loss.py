"""The dense-head and distillation loss kernels (pcp_centerhead_loss, pcp_centerhead_loss_ext, pcp_anchor_loss, pcp_distill_loss) against
the float64 references of tests/loss_refs.py, on every case of its tables.  Every tolerance is a derived bound of that file, each loss and
each gradient element against its own, nothing on top and never the largest entry.  Each comparison prints 'RATIO <group> <what> <largest
|got - ref| / bound>' (pytest -s); the groups are focal, reg, ext, anchor, distill.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import loss_refs as lr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.678                # what every float a launch must write, or must not touch, holds before it
ARG = 1                          # PCP_ERR_ARG of include/pcp_hip.h


def _mods():
    from pcp_amd import lib, train_ops
    return lib, train_ops


def _dev(a):
    a = np.asarray(a)
    return torch.from_numpy(np.array(a, dtype=np.int32 if a.dtype.kind == 'i' else np.float32)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _sent(shape):
    return torch.full(tuple(shape), SENT, dtype=torch.float32, device=DEV)


def _sent32():
    return np.float32(SENT)


def _within(group, what, got, ref, bnd):
    g = _host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert g.shape == np.shape(ref), (what, g.shape, np.shape(ref))
    r = lr.worst(g, ref, bnd)
    print('\nRATIO %-8s %-64s %.5f' % (group, what, r))
    assert r <= 1.0, '%s: |got - ref| / bound = %r' % (what, r)


def _split_head_grad(group_reg, what, dhead, ref_dhead, b_dhead, ch_hm, ncls, reg_ch, group_focal=None):
    """the heat-map channels, the regression channels, and exact zeros everywhere else; no sentinel left"""
    g = _host(dhead)
    assert not (g == _sent32()).any(), what + ': a gradient element was not written'
    hm = slice(ch_hm, ch_hm + ncls)
    _within(group_focal or group_reg, what + ' dhead heat-map channels', g[..., hm], ref_dhead[..., hm], b_dhead[..., hm])
    _within(group_reg, what + ' dhead regression channels', g[..., list(reg_ch)], ref_dhead[..., list(reg_ch)], b_dhead[..., list(reg_ch)])
    rest = [ch for ch in range(g.shape[3]) if not (ch_hm <= ch < ch_hm + ncls) and ch not in reg_ch]
    assert not g[..., rest].any() and not ref_dhead[..., rest].any(), what + ': a channel no loss term reads holds a gradient'


# ---- CenterHead, the one-head entry point ---------------------------------------------------------------------------------------------------

def _headloss_desc(lib, c, ds):
    d = lib.HeadLoss()
    d.batch, d.h, d.w, d.ld, d.ld_d, d.num_class, d.ch_hm, d.k = c.B, c.H, c.W, c.ld, c.ld_d, c.ncls, c.ch_hm, c.K
    for j in range(8):
        d.reg_ch[j], d.code_weights[j] = ds['reg_ch'][j], ds['code_weights'][j]
    d.cls_weight, d.loc_weight = ds['cls_weight'], ds['loc_weight']
    return d


@pytest.mark.parametrize('i', range(len(lr.CH_CASES)))
def test_centerhead_loss_and_every_gradient_element_within_the_bounds(i):
    lib, tops = _mods()
    c, d = lr.CH_CASES[i], lr.ch_data(i)
    ds, ref = d['desc'], d['ref']
    what = 'case %d (%d,%d,%d,%d) K=%d ld=%d/%d %s' % (i, c.B, c.H, c.W, c.ncls, c.K, c.ld, c.ld_d, c.flavour)
    desc = _headloss_desc(lib, c, ds)
    args = [_dev(d[k]) for k in ('heat', 'tb', 'inds', 'mask')]
    head = _dev(d['head'])
    dhead = _sent((c.B, c.H, c.W, c.ld_d))
    losses = _host(tops.centerhead_loss(head, desc, *args, dhead=dhead, grad_scale=c.grad_scale))
    assert losses[3] == ref['losses'][3]
    _within('focal', what + ' hm loss', losses[[0]], ref['losses'][[0]], ref['b_losses'][[0]])
    _within('reg', what + ' loc loss', losses[[1]], ref['losses'][[1]], ref['b_losses'][[1]])
    _within('focal', what + ' hm + loc', losses[[2]], ref['losses'][[2]], ref['b_losses'][[2]])
    _split_head_grad('reg', what, dhead, ref['dhead'], ref['b_dhead'], c.ch_hm, c.ncls, ds['reg_ch'], group_focal='focal')
    again = _host(tops.centerhead_loss(head, desc, *args, dhead=None, grad_scale=c.grad_scale))
    _within('focal', what + ' losses without a gradient buffer', again, ref['losses'], ref['b_losses'])
    assert torch.equal(head, _dev(d['head']))


# ---- CenterHead, several heads ------------------------------------------------------------------------------------------------------------------

def _ext_call(i, with_grad=True):
    lib, tops = _mods()
    c, d = lr.EXT_CASES[i], lr.ext_data(i)
    desc = lib.HeadLossExt()
    desc.batch, desc.h, desc.w, desc.k = c.B, c.H, c.W, c.K
    desc.cls_weight, desc.loc_weight = d['desc']['cls_weight'], d['desc']['loc_weight']
    for j, v in enumerate(d['desc']['code_weights']):
        desc.code_weights[j] = v
    heads = []
    for h in d['heads']:
        heads.append(dict(head=_dev(h['head']), heat=_dev(h['heat']), tb=_dev(h['tb']), inds=_dev(h['inds']), mask=_dev(h['mask']),
                          ch_hm=h['ch_hm'], num_class=h['num_class'], reg_ch=h['reg_ch'], dhead=_sent((c.B, c.H, c.W, h['ld_d']))))
    losses, total, dheads = tops.centerhead_loss_ext(desc, heads, with_grad=with_grad, grad_scale=c.grad_scale)
    return _host(losses).copy(), _host(total).copy(), ([_host(g).copy() for g in dheads] if with_grad else None)


@pytest.mark.parametrize('i', range(len(lr.EXT_CASES)))
def test_centerhead_loss_ext_within_the_bounds_and_the_same_bits_on_every_run(i):
    lib, _tops = _mods()
    assert lib.DET_MAX_HEADS == lr.MAX_HEADS and lib.HEADLOSS_MAX_CODES == lr.MAX_CODES
    c, d = lr.EXT_CASES[i], lr.ext_data(i)
    ref = d['ref']
    losses, total, dheads = _ext_call(i)
    assert np.array_equal(losses[:, 3], ref['losses'][:, 3])
    for hi, h in enumerate(d['heads']):
        what = 'case %d head %d ncls=%d codes=%d ld=%d/%d' % (i, hi, h['num_class'], len(h['reg_ch']), h['head'].shape[3], h['ld_d'])
        _within('ext', what + ' losses', losses[hi], ref['losses'][hi], ref['b_losses'][hi])
        _split_head_grad('ext', what, torch.from_numpy(dheads[hi]), ref['dheads'][hi], ref['b_dheads'][hi], h['ch_hm'], h['num_class'],
                         h['reg_ch'])
    _within('ext', 'case %d total' % i, total, np.array([ref['total']]), np.array([ref['b_total']]))
    t = np.float32(0)
    for v in losses[:, 2]:
        t = np.float32(t + v)
    assert total[0] == t, 'total is the float32 sum of the float32 per-head losses in head order'
    l2, t2, d2 = _ext_call(i)
    assert losses.tobytes() == l2.tobytes() and total.tobytes() == t2.tobytes(), 'a second run gave other bits'
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dheads, d2)), 'a second run gave other gradient bits'
    l3, t3, _none = _ext_call(i, with_grad=False)
    assert losses.tobytes() == l3.tobytes() and total.tobytes() == t3.tobytes(), 'the call without gradients gave other losses'


# ---- AnchorHeadSingle ---------------------------------------------------------------------------------------------------------------------------

def _anchor_desc(lib, c, ds):
    d = lib.AnchorLoss()
    d.batch, d.h, d.w, d.ld, d.ld_d = c.B, c.H, c.W, c.ld, c.ld_d
    d.anchors_per_loc, d.num_class, d.num_dir_bins = c.A, c.ncls, c.bins
    d.ch_cls, d.ch_box, d.ch_dir = 0, c.A * c.ncls, c.A * c.ncls + c.A * 7
    d.dir_offset, d.dir_period = ds['dir_offset'], ds['dir_period']
    d.cls_weight, d.loc_weight, d.dir_weight = ds['cls_weight'], ds['loc_weight'], ds['dir_weight']
    for j in range(7):
        d.code_weights[j] = ds['code_weights'][j]
    return d


@pytest.mark.parametrize('i', range(len(lr.AN_CASES)))
def test_anchor_loss_and_all_three_gradient_groups_within_the_bounds(i):
    lib, tops = _mods()
    c, d = lr.AN_CASES[i], lr.an_data(i)
    ref, grp = d['ref'], d['ref']['groups']
    what = 'case %d (%d,%d,%d) A=%d ncls=%d bins=%d ld=%d/%d gs=%g' % (i, c.B, c.H, c.W, c.A, c.ncls, c.bins, c.ld, c.ld_d, c.grad_scale)
    desc = _anchor_desc(lib, c, d['desc'])
    head, anchors, labels, reg = _dev(d['head']), _dev(d['anchors']), _dev(d['labels']), _dev(d['reg'])
    dhead = _sent((c.B, c.H, c.W, c.ld_d))
    losses = _host(tops.anchor_loss(head, anchors, labels, reg, desc, dhead=dhead, grad_scale=c.grad_scale))
    assert losses[4] == ref['losses'][4]
    for j, name in enumerate(('cls', 'loc', 'dir', 'total')):
        _within('anchor', '%s %s loss' % (what, name), losses[[j]], ref['losses'][[j]], ref['b_losses'][[j]])
    g = _host(dhead)
    assert not (g == _sent32()).any(), 'a gradient element was not written'
    for name in ('cls', 'box', 'dir'):
        if name == 'dir' and not c.bins:
            continue
        _within('anchor', '%s %s gradient' % (what, name), g[..., grp[name]], ref['dhead'][..., grp[name]], ref['b_dhead'][..., grp[name]])
    assert grp['pad'].stop - grp['pad'].start == c.ld_d - c.A * (c.ncls + 7 + c.bins) and not g[..., grp['pad']].any()
    again = _host(tops.anchor_loss(head, anchors, labels, reg, desc, dhead=None, grad_scale=c.grad_scale))
    _within('anchor', what + ' losses without a gradient buffer', again, ref['losses'], ref['b_losses'])


@pytest.mark.parametrize('field,value', [('num_class', 17), ('num_dir_bins', 9)])
def test_anchor_loss_refuses_what_its_register_arrays_cannot_hold(field, value):
    lib, tops = _mods()
    c, d = lr.AN_CASES[0], lr.an_data(0)
    desc = _anchor_desc(lib, c, d['desc'])
    setattr(desc, field, value)
    desc.ld = desc.ld_d = 512
    head = torch.zeros((c.B, c.H, c.W, 512), device=DEV)
    dhead, losses = _sent((c.B, c.H, c.W, 512)), _sent((5,))
    L, p = lib.load(), tops._p
    ws = tops._anchor_ws(head.device, L.pcp_anchor_loss_workspace_bytes(c.B))
    st = L.pcp_anchor_loss(ctypes.byref(desc), p(head), p(_dev(d['anchors'])), p(_dev(d['labels'])), p(_dev(d['reg'])), 0.5, p(ws), ws.numel(),
                           p(losses), p(dhead), tops._stream())
    torch.cuda.synchronize()
    assert st == ARG
    assert bool((dhead == SENT).all()) and bool((losses == SENT).all())


# ---- distillation -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', range(len(lr.DS_CASES)))
def test_distill_loss_and_gradient_within_the_bounds(i):
    _lib, tops = _mods()
    c, d = lr.DS_CASES[i], lr.ds_data(i)
    ref = d['ref']
    what = 'c=%d pixels=%d weight=%g gs=%g acc=%d' % (c.c, c.pixels, c.weight, c.grad_scale, c.accumulate)
    fused, early = _dev(d['fused']), _dev(d['early'])                      # 1e30 beyond c: never read into the result
    dfused = _sent((c.pixels, c.c + 2))
    if c.accumulate:
        dfused[:, :c.c] = _dev(d['prior'][:, :c.c])
    loss = _host(tops.distill_loss(fused, early, c.c, weight=c.weight, dfused=dfused, accumulate=c.accumulate, grad_scale=c.grad_scale))
    _within('distill', what + ' loss', loss, np.array([ref['loss']]), np.array([ref['b_loss']]))
    g = _host(dfused)
    assert (g[:, c.c:] == _sent32()).all(), 'a column beyond c was written'
    assert not (g[:, :c.c] == _sent32()).any() and np.isfinite(g[:, :c.c]).all()
    _within('distill', what + ' dfused', g[:, :c.c], ref['dfused'], ref['b_dfused'])
    again = _host(tops.distill_loss(fused, early, c.c, weight=c.weight))
    assert again.tobytes() == loss.tobytes(), 'the loss without a gradient buffer has other bits'


def test_distill_refuses_more_channels_than_a_wave_holds():
    lib, tops = _mods()
    L, p = lib.load(), tops._p
    c = lr.DIST_MAX_C + 1
    fused, early = torch.zeros((3, c), device=DEV), torch.zeros((3, c), device=DEV)
    loss, dfused = _sent((1,)), _sent((3, c))
    st = L.pcp_distill_loss(p(fused), c, p(early), c, 3, c, 10.0, 1.0, p(tops._loss_ws(fused.device)), p(loss), p(dfused), c, 0, tops._stream())
    torch.cuda.synchronize()
    assert st == ARG
    assert bool((loss == SENT).all()) and bool((dfused == SENT).all())
