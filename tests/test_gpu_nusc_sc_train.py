"""SC backbone training on MI355X: pcp_avgpool_nhwc_backward, pcp_sc_gate_backward, pcp_add_relu / pcp_add_relu_backward against torch CPU
autograd, one _SCBottleneckTrain and the whole SCConvBackbone2dStride4 against the reference's own modules (fixtures g22_sc_block_train and
g22_sc_backbone_train, tests/golden/make_golden_nusc_sc_train.py), pointpillar_jr_nomap end to end (a step repeats bit for bit, the bf16 loop tracks the fp32
loss, eval after a step), and the refusals."""
import ctypes
import json
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nusc_sc_refs as refs
from helpers import load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL, RTOL = 1e-6, 1e-5          # a handful of fp32 operations per element
PCP_ERR_ARG = 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def _window(t, ld, off, fill=7.0):
    """(B, H, W, c) CPU tensor -> (B, H, W, ld) device buffer holding it at channel offset `off`, `fill` elsewhere"""
    buf = torch.full(t.shape[:3] + (ld,), fill, dtype=torch.float32)
    buf[..., off:off + t.shape[3]] = t
    return buf.to(DEV)


def _close(got, want, what):
    got, want = got.cpu(), want.cpu()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print('%s: max err %.3e' % (what, float(err.max())))
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- op tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [4, 16])
@pytest.mark.parametrize('h,w,sh,sw,r', refs.SHAPES)
def test_avgpool_backward_matches_autograd(h, w, sh, sw, r, c):
    from pcp_amd import train_ops as tops
    g = _gen(h * 1000 + w * 10 + c)
    x = _rand(g, 2, c, h, w).requires_grad_(True)
    dp = _rand(g, 2, c, sh, sw)
    F.avg_pool2d(x, r, r).backward(dp)
    want = _nhwc(x.grad)
    dp_buf = _window(_nhwc(dp), c + 8, 4)
    # overwriting: the window is written, the dropped remainder rows / columns exactly 0, the rest of the buffer untouched
    dx = _window(torch.zeros(2, h, w, c), c + 12, 8)
    dx[..., 8:8 + c] = float('nan')
    tops.avgpool_nhwc_backward(dp_buf, r, dx, c, dpooled_ch_off=4, dx_ch_off=8)
    got = dx.cpu()
    _close(got[..., 8:8 + c], want, 'pool backward')
    assert bool((got[:, sh * r:, :, 8:8 + c] == 0).all()) and bool((got[:, :, sw * r:, 8:8 + c] == 0).all())
    assert bool((got[..., :8] == 7.0).all()) and bool((got[..., 8 + c:] == 7.0).all())
    # accumulating: base + gradient; the remainder keeps the base bit for bit
    base = _rand(g, 2, h, w, c)
    dx = _window(base, c + 12, 8)
    tops.avgpool_nhwc_backward(dp_buf, r, dx, c, accumulate=True, dpooled_ch_off=4, dx_ch_off=8)
    got = dx.cpu()
    _close(got[..., 8:8 + c], base + want, 'pool backward, accumulating')
    assert torch.equal(got[:, sh * r:, :, 8:8 + c], base[:, sh * r:]) and torch.equal(got[:, :, sw * r:, 8:8 + c], base[:, :, sw * r:])
    assert bool((got[..., :8] == 7.0).all()) and bool((got[..., 8 + c:] == 7.0).all())


@pytest.mark.parametrize('c', [4, 16])
@pytest.mark.parametrize('h,w,sh,sw,r', refs.SHAPES)
def test_sc_gate_backward_matches_autograd(h, w, sh, sw, r, c):
    from pcp_amd import train_ops as tops
    g = _gen(h * 1000 + w * 10 + c + 1)
    t = _rand(g, 2, c, h, w).requires_grad_(True)
    x = _rand(g, 2, c, h, w).requires_grad_(True)
    s = _rand(g, 2, c, sh, sw).requires_grad_(True)
    dout = _rand(g, 2, c, h, w)
    (t * torch.sigmoid(x + F.interpolate(s, size=(h, w)))).backward(dout)
    t_b, x_b, s_b = _window(_nhwc(t.detach()), c + 4, 4), _window(_nhwc(x.detach()), 2 * c + 8, c), _window(_nhwc(s.detach()), c + 8, 8)
    do_b = _window(_nhwc(dout), c + 4, 0)
    dt_b = _window(torch.zeros(2, h, w, c), c + 8, 4)
    dz_b = _window(torch.zeros(2, h, w, c), c + 4, 4)
    ds_b = _window(torch.zeros(2, sh, sw, c), c + 12, 4)
    base = _rand(g, 2, h, w, c)
    dx_b = _window(base, c + 8, 0)
    tops.sc_gate_backward(do_b, t_b, x_b, s_b, c, dt=dt_b, dz=dz_b, dx=dx_b, accumulate_dx=True, ds=ds_b, t_ch_off=4, x_ch_off=c, s_ch_off=8,
                          dt_ch_off=4, dz_ch_off=4, ds_ch_off=4)
    _close(dt_b[..., 4:4 + c], _nhwc(t.grad), 'dt')
    _close(dz_b[..., 4:4 + c], _nhwc(x.grad), 'dz')
    _close(dx_b[..., :c], base + _nhwc(x.grad), 'dx, accumulating')
    _close(ds_b[..., 4:4 + c], _nhwc(s.grad), 'ds')
    for buf, lo, hi in ((dt_b, 4, 4 + c), (dz_b, 4, 4 + c), (ds_b, 4, 4 + c), (dx_b, 0, c)):
        assert bool((buf[..., :lo] == 7.0).all()) and bool((buf[..., hi:] == 7.0).all())
    # dt in place over dout, dx overwritten, dz / ds allocated: the same bits
    dx2 = _window(torch.zeros(2, h, w, c), c + 8, 0)
    dt2, dz2, ds2 = tops.sc_gate_backward(do_b, t_b, x_b, s_b, c, dx=dx2, t_ch_off=4, x_ch_off=c, s_ch_off=8)
    assert dt2 is do_b and torch.equal(dt2[..., :c], dt_b[..., 4:4 + c]) and torch.equal(dz2, dz_b[..., 4:4 + c].contiguous())
    assert torch.equal(ds2, ds_b[..., 4:4 + c].contiguous()) and torch.equal(dx2[..., :c], dz2)


@pytest.mark.parametrize('c', [4, 16])
def test_add_relu_and_its_backward_match_autograd(c):
    from pcp_amd import train_ops as tops
    g = _gen(77 + c)
    h, w = 7, 5
    z = _rand(g, 2, h, w, c).requires_grad_(True)
    res = _rand(g, 2, h, w, c)
    dout = _rand(g, 2, h, w, c)
    out = torch.relu(z + res)
    out.backward(dout)
    z_b, r_b, o_b = _window(z.detach(), c + 4, 4), _window(res, c + 8, 0), _window(torch.zeros(2, h, w, c), c + 4, 0)
    tops.add_relu(z_b, r_b, c, out=o_b, z_ch_off=4)
    _close(o_b[..., :c], out.detach(), 'relu(z + res)')
    assert bool((o_b[..., c:] == 7.0).all())
    tops.add_relu(z_b, r_b, c, z_ch_off=4)                                      # in place over z
    assert torch.equal(z_b[..., 4:], o_b[..., :c]) and bool((z_b[..., :4] == 7.0).all())
    d_b = _window(dout, c + 8, 4)
    dz2 = _window(torch.zeros(2, h, w, c), c + 4, 4)
    tops.add_relu_backward(d_b, o_b, c, dz2=dz2, dout_ch_off=4, dz2_ch_off=4)    # in place over dout, with a second copy
    _close(d_b[..., 4:4 + c], z.grad, 'mask backward')
    assert torch.equal(d_b[..., 4:4 + c], dz2[..., 4:]) and bool((d_b[..., :4] == 7.0).all()) and bool((dz2[..., :4] == 7.0).all())
    assert bool((d_b[..., 4 + c:] == 7.0).all())


def test_argument_checks_refuse_odd_channel_counts_and_misaligned_windows():
    from pcp_amd import lib
    L = lib.load()
    buf = torch.zeros(2, 8, 8, 16, device=DEV)
    small = torch.zeros(2, 2, 2, 16, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for c, off in ((6, 0), (4, 2)):               # c % 4 != 0; a window that starts 8 bytes into a pixel
        assert L.pcp_avgpool_nhwc_backward(p(small, off), 16, 2, 8, 8, c, 4, p(buf), 16, 0, st) == PCP_ERR_ARG
        assert L.pcp_avgpool_nhwc_backward(p(small), 16, 2, 8, 8, c, 4, p(buf, off), 16, 0, st) == PCP_ERR_ARG
        assert L.pcp_sc_gate_backward(p(buf, off), 16, p(buf), 16, p(buf), 16, p(small), 16, 2, 2, p(buf, 4), 16, p(buf, 8), 16, None, 0, 0,
                                      p(small, 4), 16, 2, 8, 8, c, st) == PCP_ERR_ARG
        assert L.pcp_sc_gate_backward(p(buf), 16, p(buf), 16, p(buf), 16, p(small), 16, 2, 2, p(buf, 4), 16, p(buf, 8), 16, None, 0, 0,
                                      p(small, 4 + off), 16, 2, 8, 8, c, st) == PCP_ERR_ARG
        assert L.pcp_add_relu(p(buf, off), 16, p(buf), 16, p(buf, 8), 16, 128, c, st) == PCP_ERR_ARG
        assert L.pcp_add_relu_backward(p(buf), 16, p(buf), 16, p(buf, 8 + off), 16, None, 0, 128, c, st) == PCP_ERR_ARG
    assert L.pcp_avgpool_nhwc_backward(p(small), 18, 2, 8, 8, 4, 4, p(buf), 16, 0, st) == PCP_ERR_ARG       # ld % 4 != 0
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0 and float(small.abs().max()) == 0.0                               # nothing was launched


# ---- one bottleneck against the reference's own -----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def g22b():
    return load_golden('g22_sc_block_train.npz')


@pytest.mark.parametrize('tag', ['p32', 'p64'])
def test_bottleneck_forward_and_backward_match_the_reference(g22b, tag):
    from pcdet.models.backbones_2d.sc_conv_backbone import SCBottleneck
    from pcdet.models.train_path import _SCBottleneckTrain
    from pcp_amd import ops
    from pcp_amd.train_layers import Act, StepClock, flush_batches_tracked
    g, c = g22b, g22b['meta']['cases'][tag]
    n = int(np.prod(c['shape']))
    x_np = synth.uniform(c['seed'], c['x']['stream'], n, c['x']['lo'], c['x']['hi']).reshape(c['shape'])
    d_np = synth.uniform(c['seed'], c['dout']['stream'], n, c['dout']['lo'], c['dout']['hi']).reshape(c['shape'])
    digest = g[tag + '/x_digest']
    assert abs(float(x_np.astype(np.float64).sum()) - digest[0]) <= 1e-9 * abs(digest[0]) and float(np.abs(x_np).max()) == digest[1]
    blk = SCBottleneck(c['planes'], c['planes'], partial(torch.nn.BatchNorm2d, eps=c['bn_eps'], momentum=c['bn_momentum']))
    st = synth.fill_state_dict(c['state_shapes'], scheme=c['scheme'])
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    blk = blk.to(DEV).train()
    StepClock.tick()
    tr = _SCBottleneckTrain(blk, tag)
    x = ops.as_nhwc(torch.from_numpy(x_np).to(DEV))
    out = tr.forward(Act(x))
    got_out = out.t.permute(0, 3, 1, 2).cpu().numpy()
    err = float(np.abs(got_out - g[tag + '/out']).max())
    print('%s: output max err %.3e' % (tag, err))
    dx = tr.backward(Act(ops.as_nhwc(torch.from_numpy(d_np).to(DEV))))
    flush_batches_tracked()
    assert err <= 1e-4, err
    got = {k: p.grad.cpu().numpy() for k, p in blk.named_parameters()}
    got['input'] = dx.t.permute(0, 3, 1, 2).cpu().numpy()
    want = {k: g['%s/g/%s' % (tag, k)] for k in c['param_names']}
    want['input'] = g[tag + '/dx']
    assert set(got) == set(want)
    gmax = max(float(np.abs(v).max()) for v in want.values())
    num = den = 0.0
    for k, ref in want.items():
        scale = max(float(np.abs(ref).max()), 1e-4 * gmax)
        e = float(np.abs(got[k] - ref).max())
        print('%s %s: max err %.3e of scale %.3e' % (tag, k, e, scale))
        assert e <= 3e-2 * scale, (k, e, scale)
        num += float(((got[k].astype(np.float64) - ref) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
    print('%s: global relative L2 %.3e' % (tag, (num / den) ** 0.5))
    assert num <= (2e-2 ** 2) * den, (num / den) ** 0.5
    sd = blk.state_dict()
    for k in sd:
        if 'running_' in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), g['%s/bn/%s' % (tag, k)], rtol=2e-4, atol=0, err_msg=k)
        elif 'num_batches_tracked' in k:
            assert int(sd[k]) == int(g['%s/bn/%s' % (tag, k)]), k


# ---- the whole backbone against the reference's own ---------------------------------------------------------------------------------------

def test_stride4_backbone_forward_and_backward_match_the_reference():
    """SCConvBackbone2dStride4 alone (fixture g22_sc_backbone_train): the layers above the block -- the two windows of the merged map, the
    conv_skip + main_pass.0 fan-in, conv_out's own BatchNorm eps / momentum -- at the tolerances of the block test"""
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.sc_conv_backbone import SCConvBackbone2dStride4
    from pcp_amd import ops
    from pcp_amd.train_layers import Act
    g = load_golden('g22_sc_backbone_train.npz')
    meta = g['meta']
    n = int(np.prod(meta['canvas']))
    x_np = synth.uniform(meta['seed'], meta['x']['stream'], n, meta['x']['lo'], meta['x']['hi']).reshape(meta['canvas'])
    d_np = synth.uniform(meta['seed'], meta['dout']['stream'], g['out'].size, meta['dout']['lo'], meta['dout']['hi']).reshape(g['out'].shape)
    digest = g['x_digest']
    assert abs(float(x_np.astype(np.float64).sum()) - digest[0]) <= 1e-9 * abs(digest[0]) and float(np.abs(x_np).max()) == digest[1]
    bb = SCConvBackbone2dStride4(EasyDict(meta['cfg']), meta['input_channels'])
    st = synth.fill_state_dict(meta['state_shapes'], scheme=meta['scheme'])
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    bb = bb.to(DEV).train()
    d = bb({'spatial_features': torch.from_numpy(x_np).to(DEV)})
    err = float(np.abs(d['spatial_features_2d'].cpu().numpy() - g['out']).max())
    print('backbone output max err %.3e' % err)
    (_name, backward), = d['_pcp_tape']
    dx = backward(Act(ops.as_nhwc(torch.from_numpy(d_np).to(DEV))))
    assert err <= 1e-4, err
    cap = meta['whole_cap']

    def sample(t):
        a = t.detach().reshape(-1)
        return (a if a.numel() <= cap else a[::a.numel() // 1024][:1024]).cpu().numpy()
    names = meta['param_names']
    params = dict(bb.named_parameters())
    got = {k: sample(params[k].grad) for k in names}
    want = {k: g['g/' + k] for k in names}
    got['input'], want['input'] = dx.t.float().permute(0, 3, 1, 2).cpu().numpy(), g['dx']
    gmax = max(float(np.abs(v).max()) for v in want.values())
    num = den = 0.0
    worst = (0.0, '')
    for k, ref in want.items():
        scale = max(float(np.abs(ref).max()), 1e-4 * gmax)
        e = float(np.abs(got[k] - ref).max())
        worst = max(worst, (e / scale, k))
        assert e <= 3e-2 * scale, (k, e, scale)
        num += float(((got[k].astype(np.float64) - ref) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
    print('backbone gradients: global relative L2 %.3e; worst tensor %.3e of its scale at %s' % ((num / den) ** 0.5, worst[0], worst[1]))
    assert num <= (2e-2 ** 2) * den, (num / den) ** 0.5
    nmax = float(g['grad_digest'][:, 0].max())
    for i, k in enumerate(names):                                                 # the whole tensors, through their norms
        ref = g['grad_digest'][i]
        mine = float(params[k].grad.double().norm())
        assert abs(mine - ref[0]) <= 2e-2 * max(ref[0], 1e-4 * nmax), (k, mine, ref[0])
    sd = bb.state_dict()
    for k in sd:
        if 'running_' in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), g['bn/' + k], rtol=2e-4, atol=0, err_msg=k)
        elif 'num_batches_tracked' in k:
            assert int(sd[k]) == int(g['bn/' + k]), k


# ---- pointpillar_jr_nomap itself --------------------------------------------------------------------------------------------------------
# No reference values at this level: no whole-model fixture could be conditioned (the generator's docstring).  The model runs on the 60 x 60 mini
# grid of g20_nusc_mini (stem 30 -> pooled 7, main pass 15 -> pooled 3) with that fixture's weights and cloud and seeded 10-column boxes.

@pytest.fixture(scope='module')
def g22m():
    import os
    from pcdet.config import EasyDict, cfg_from_yaml_file
    g = load_golden('g20_nusc_mini.npz')
    meta = dict(g['meta']['cases']['nomap'])
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml = os.path.join(repo, 'practical-collab-perception_amd', 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_nomap.yaml')
    meta['optimization'] = cfg_from_yaml_file(yaml, EasyDict()).OPTIMIZATION
    meta['total_it_each_epoch'] = 5
    return dict(meta=meta, points=g['points'], gt_boxes=refs.sc_model_gt(300, meta['pc_range'][3]))


def _model_and_optimizer(g):
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, 'practical-collab-perception_amd', 'tools'))
    from train_utils.optimization import build_optimizer, build_scheduler
    from pcdet.config import EasyDict
    from pcdet.models import build_network_from_meta
    meta = g['meta']
    model = build_network_from_meta(meta)
    st = synth.fill_state_dict(meta['state_shapes'], scheme=meta['weight_scheme'])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(DEV)
    ocfg = EasyDict(meta['optimization'])
    opt = build_optimizer(model, ocfg)
    sched, _ = build_scheduler(opt, meta['total_it_each_epoch'], ocfg.NUM_EPOCHS, -1, ocfg)
    return model, opt, sched, ocfg


def _model_batch(g):
    return {'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}],
            'gt_boxes': torch.from_numpy(g['gt_boxes']).to(DEV)}


def _model_first_step(g):
    model, opt, sched, _ocfg = _model_and_optimizer(g)
    sched.step(0)
    model.train()
    opt.zero_grad()
    ret, _tb, _disp = model(_model_batch(g))
    model.update_global_step()
    ret['loss'].backward()
    return float(ret['loss'].detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, (model, opt)


@pytest.fixture(scope='module')
def model_fp32_step(g22m):
    return _model_first_step(g22m)


def test_model_train_step_repeats_bit_for_bit(g22m, model_fp32_step):
    la, ga, (model, _opt) = model_fp32_step
    lb, gb, _ = _model_first_step(g22m)
    assert np.isfinite(la) and la == lb and set(ga) == set(gb) == set(n for n, p in model.named_parameters() if p.requires_grad)
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for n, v in ga.items() if n.startswith('backbone_2d.'))
    assert not [n for n in ga if not torch.equal(ga[n], gb[n])]


def test_model_bf16_loop_iteration_tracks_the_fp32_loss(g22m, model_fp32_step, monkeypatch):
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    l16, g16, _ = _model_first_step(g22m)
    l32 = model_fp32_step[0]
    print('bf16 loop loss %.6f, fp32 %.6f' % (l16, l32))
    assert np.isfinite(l16) and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert all(torch.isfinite(v).all() for v in g16.values())


def test_eval_after_a_train_step_uses_the_stepped_weights(g22m):
    """the packed inference cache is dropped by the training forward and the BatchNorm counters are flushed: after one optimizer step,
    eval() gives the bits of a fresh model loaded from the stepped state_dict()"""
    from pcdet.models import build_network_from_meta
    g = g22m
    _l, _g, (model, opt) = _model_first_step(g)
    opt.step()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    st0 = synth.fill_state_dict(g['meta']['state_shapes'], scheme=g['meta']['weight_scheme'])
    counters = [k for k in sd if k.startswith('backbone_2d.') and k.endswith('num_batches_tracked')]
    assert len(counters) == 47 and all(int(sd[k]) == int(st0[k]) + 1 for k in counters)          # 6 blocks x 7 + 5 BatchNorms, one forward each

    def eval_map(m):
        m.eval()
        batch = {'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}]}
        with torch.no_grad():
            m(batch)
        return batch['spatial_features_2d'].clone()
    got = eval_map(model)
    fresh = build_network_from_meta(g['meta'])
    fresh.load_state_dict(sd)
    want = eval_map(fresh.to(DEV))
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_a_main_pass_map_below_the_pool_size_is_refused(g22m):
    from pcdet.models import build_network_from_meta
    bb = build_network_from_meta(g22m['meta']).backbone_2d.to(DEV).train()
    with pytest.raises(NotImplementedError, match='POOLING_R'):
        bb({'spatial_features': torch.zeros(1, 64, 8, 8, device=DEV)})
    with pytest.raises(ValueError, match='even stem sizes'):
        bb({'spatial_features': torch.zeros(1, 64, 36, 34, device=DEV)})


def test_stride1_backbone_trains_through_the_same_path():
    """SCConvBackbone2dStride1 (no config of the reference uses it): a forward + backward is finite, reaches every parameter and repeats"""
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.sc_conv_backbone import SCConvBackbone2dStride1
    meta = load_golden('g20_nusc_mini.npz')['meta']['cases']['stride1']
    bb = SCConvBackbone2dStride1(EasyDict(meta['cfg']), meta['input_channels'])
    st = synth.fill_state_dict(meta['state_shapes'], scheme='he')
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    bb = bb.to(DEV).train()
    canvas = torch.from_numpy(synth.uniform(5, 1, 2 * 64 * 20 * 24, 0.0, 1.0).reshape(2, 64, 20, 24)).to(DEV)
    dout = torch.from_numpy(synth.uniform(5, 2, 2 * 20 * 24 * 128, -1.0, 1.0).reshape(2, 20, 24, 128)).to(DEV)
    runs = []
    for _ in range(2):
        bb.zero_grad()
        d = bb({'spatial_features': canvas})
        assert tuple(d['spatial_features_2d'].shape) == (2, 128, 20, 24)
        (name, backward), = d['_pcp_tape']
        from pcp_amd.train_layers import Act
        dx = backward(Act(dout.clone()))
        runs.append((d['spatial_features_2d'].clone(), dx.t.clone(), {n: p.grad.clone() for n, p in bb.named_parameters()}))
    assert name == 'backbone_2d' and tuple(runs[0][1].shape) == (2, 20, 24, 64)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in bb.parameters())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
