"""Training PillarFeatureNet at any raw width on MI355X: pcp_pfn_train_features_w against the four fixed-width kernels (bit for bit) and its
argument checks, VFETrain against the reference's own DynamicPillarVFE under autograd at raw widths 10, 7 and 12 (fixture
g23_vfe_train_widths, tests/golden/make_golden_nusc_vfe_train.py), pointpillar_jr_withmap end to end on the mini grid of g20_nusc_mini (a
step repeats bit for bit, the bf16 loop tracks the fp32 loss, eval after a step) and the refusal of the other compositions."""
import ctypes

import numpy as np
import pytest
import torch

import nusc_sc_refs as refs
from helpers import load_golden
from pcp_amd import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PCP_OK, PCP_ERR_ARG = 0, 1


def _close(got, want, tol, what):
    """the comparison of tests/test_gpu_train_ops.py: max error against the reference's scale"""
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().float().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-6)
    print('%s: max err %.3e of scale %.3e' % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


@pytest.fixture(scope='module')
def g23():
    return load_golden('g23_vfe_train_widths.npz')


def _vfe(meta, num_raw, use_abs=True, with_dist=False, filters=(64, 64), use_norm=True):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE
    cfg = EasyDict(NAME='DynPillarVFE', WITH_DISTANCE=with_dist, USE_ABSLOTE_XYZ=use_abs, USE_NORM=use_norm, NUM_FILTERS=list(filters))
    return DynamicPillarVFE(model_cfg=cfg, num_point_features=num_raw, voxel_size=meta['voxel_size'], grid_size=meta['grid_size'],
                            point_cloud_range=meta['pc_range'])


def _pillarised(g23, tag='w12'):
    """the crowded 13-column cloud of case w12 on the device, pillarised with the reproducible row order VFETrain uses"""
    from pcp_amd import ops
    meta = g23['meta']
    pts = torch.from_numpy(g23[tag + '/points']).to(DEV)
    grid = ops.make_grid(meta['pc_range'], meta['voxel_size'], meta['grid_size'], 2)
    vox = ops.voxelize(pts, grid, want_inverse=False, want_counts=False)
    ops.voxelize_sort_pillar_rows(vox)
    return pts, vox


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num_raw,fw', [(5, 16), (11, 32)])
def test_run_time_width_kernel_gives_the_bits_of_the_fixed_width_kernels(g23, num_raw, fw):
    """widths 5 (16-float rows) and 11 (32-float rows) of a 13-float point row, on the cloud with cells of 16 .. 1500 points: fbuf and
    slot_pillar of pcp_pfn_train_features_w equal those of k_pfnt_feat<5> / <11> bit for bit, padding and untouched rows included"""
    from pcp_amd import train_ops as tops
    pts, vox = _pillarised(g23)
    P, Nk = (int(v) for v in vox.counters[:2].tolist())
    n = pts.shape[0]
    assert vox.row_stride == 13 and 0 < Nk < n and P == g23['meta']['cases']['w12']['pillars']     # some rows are out of range: never written
    out = []
    for fn in (tops.pfn_train_features, tops.pfn_train_features_w):
        fbuf = torch.full((n, fw), 7.0, dtype=torch.float32, device=DEV)
        sp = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        fn(pts, vox, num_raw, fbuf, sp)
        out.append((fbuf, sp))
    torch.cuda.synchronize()
    (fa, sa), (fb, sb) = out
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)) and torch.equal(sa, sb)
    assert bool((fb[:Nk, num_raw + 6:] == 0).all()) and bool((fb[Nk:] == 7.0).all()) and bool((sb[Nk:] == -7).all())
    assert int(sb[:Nk].min()) == 0 and int(sb[:Nk].max()) == P - 1 and bool((sb[1:Nk] >= sb[:Nk - 1]).all())      # bucket order
    assert float(fb[:Nk, :num_raw + 6].abs().max()) > 0


def test_default_case_of_the_fixed_width_entry_forwards_to_the_run_time_kernel(g23):
    """pcp_pfn_train_features at a width without a kernel of its own (10 -> 16-float rows, 12 -> 32-float rows) gives what the new entry
    gives; above 26 columns it returns PCP_ERR_ARG and writes nothing"""
    from pcp_amd import lib, train_ops as tops
    pts, vox = _pillarised(g23)
    n = pts.shape[0]
    for num_raw, fw in ((10, 16), (12, 32)):
        a, b = (torch.full((n, fw), 7.0, dtype=torch.float32, device=DEV) for _ in range(2))
        sa, sb = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
        tops.pfn_train_features(pts, vox, num_raw, a, sa)
        tops.pfn_train_features_w(pts, vox, num_raw, b, sb)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(sa, sb) and int(sa.max()) > 0
    wide = torch.zeros((64, 40), dtype=torch.float32, device=DEV)
    buf = torch.full((64, 32), 7.0, dtype=torch.float32, device=DEV)
    sp = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.load().pcp_pfn_train_features(p(wide), 64, 40, 27, ctypes.byref(vox.grid), p(vox.workspace), p(buf), p(sp), st) == PCP_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((sp == -7).all())


def test_argument_checks_return_err_arg_without_launching(g23):
    from pcp_amd import lib
    L = lib.load()
    pts, vox = _pillarised(g23)
    n = pts.shape[0]
    fbuf = torch.full((n, 32), 7.0, dtype=torch.float32, device=DEV)
    sp = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G, W = ctypes.byref(vox.grid), p(vox.workspace)

    def call(points=p(pts), rows=n, stride=13, num_raw=10, fw=16, grid=G, ws=W, out=p(fbuf), slots=p(sp)):
        return L.pcp_pfn_train_features_w(points, rows, stride, num_raw, fw, grid, ws, out, slots, st)
    bad = [dict(num_raw=2), dict(num_raw=27, stride=28, fw=32), dict(num_raw=0), dict(num_raw=-1),          # width outside 3 .. 26
           dict(num_raw=12, stride=12), dict(stride=10), dict(stride=0),                                    # row shorter than 1 + num_raw
           dict(fw=8), dict(fw=24), dict(fw=64), dict(fw=0), dict(fw=17),                                   # fw is 16 or 32
           dict(num_raw=11, fw=16), dict(num_raw=12, fw=16),                                                # num_raw + 6 > fw
           dict(rows=-1), dict(points=None), dict(grid=None), dict(ws=None), dict(out=None), dict(slots=None)]
    for kw in bad:
        assert call(**kw) == PCP_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((fbuf == 7.0).all()) and bool((sp == -7).all())                                             # nothing was launched
    # the edges of the accepted range
    assert call(rows=0) == PCP_OK
    for num_raw, fw in ((3, 16), (10, 16), (10, 32), (11, 32), (12, 32)):
        assert call(num_raw=num_raw, fw=fw) == PCP_OK, (num_raw, fw)
    torch.cuda.synchronize()
    assert int(sp.max()) > 0


def test_width_26_fills_the_whole_32_float_row():
    """the widest row: 26 raw columns + 6 derived ones, no padding; a small cloud with a pillar of three points and rows out of range"""
    from pcp_amd import ops, train_ops as tops
    n, nr = 40, 26
    pts = synth.uniform(7, 1, n * (1 + nr), -1.0, 1.0).reshape(n, 1 + nr).copy()
    pts[:, 0] = np.arange(n) % 2
    pts[:, 1:3] = synth.uniform(7, 2, n * 2, -1.7, 1.5).reshape(n, 2)             # range +-1.6: some rows fall outside
    pts[1, 1:3], pts[3, 1:3], pts[5, 1:3] = (0.31, -0.52), (0.33, -0.55), (0.39, -0.41)          # frame 1, cell (9, 5): a pillar of three
    pc_range, voxel = [-1.6, -1.6, -1.0, 1.6, 1.6, 1.0], [0.2, 0.2, 2.0]
    grid = ops.make_grid(pc_range, voxel, [16, 16, 1], 2)
    dpts = torch.from_numpy(pts).to(DEV)
    vox = ops.voxelize(dpts, grid, want_inverse=False, want_counts=False)
    ops.voxelize_sort_pillar_rows(vox)
    P, Nk = (int(v) for v in vox.counters[:2].tolist())
    fbuf = torch.full((n, 32), 7.0, dtype=torch.float32, device=DEV)
    sp = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tops.pfn_train_features_w(dpts, vox, nr, fbuf, sp)
    got, slot = fbuf.cpu().numpy(), sp.cpu().numpy()
    assert 0 < Nk < n and P <= Nk - 2
    # every kept row appears once, raw columns verbatim; the derived columns from float64 statements of the same row
    ij = np.floor((pts[:, 1:3].astype(np.float64) - (-1.6)) / 0.2)
    keep = np.nonzero(((ij >= 0) & (ij < 16)).all(1))[0]
    assert keep.size == Nk
    order = [int(np.nonzero((pts[:, 1:] == got[s, :nr]).all(1))[0][0]) for s in range(Nk)]
    assert sorted(order) == sorted(keep.tolist())
    for s, r in enumerate(order):
        mates = [order[t] for t in range(Nk) if slot[t] == slot[s]]
        mean = pts[mates, 1:4].astype(np.float64).mean(0)
        centre = np.array([ij[r, 0] * 0.2 + 0.1 - 1.6, ij[r, 1] * 0.2 + 0.1 - 1.6, 0.0])
        want = np.concatenate([pts[r, 1:4] - mean, pts[r, 1:4] - centre])
        np.testing.assert_allclose(got[s, nr:], want, rtol=0, atol=1e-6)
    assert (got[Nk:] == 7.0).all()


# ---- VFETrain against the reference's own module ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['w10', 'w7', 'w12'])
def test_vfe_train_forward_and_backward_match_the_reference(g23, tag):
    """raw widths 10 (F = 16, no padding), 7 (F = 13 in 16-float rows) and 12 (F = 18 in 32-float rows): voxel_coords exactly;
    pillar_features (2e-5), running statistics (1e-5) and the six parameter gradients (5e-4) at the tolerances of
    test_vfe_train_forward_backward_matches_autograd.  Before pcp_pfn_train_features_w: NotImplementedError in the train-mode forward."""
    from pcdet.models.train_path import VFETrain
    from pcp_amd import train_layers as tl
    meta, c = g23['meta'], g23['meta']['cases'][tag]
    vfe = _vfe(meta, c['num_raw'])
    st = synth.fill_state_dict(c['state_shapes'], scheme=c['scheme'])
    vfe.load_state_dict({k[len('vfe.'):]: torch.from_numpy(v) for k, v in st.items()})
    vfe = vfe.to(DEV).train()
    assert vfe.train_fused and not vfe.fused
    assert vfe.pfn_layers[0].norm.eps == c['bn_eps'] and vfe.pfn_layers[0].norm.momentum == c['bn_momentum']
    tl.StepClock.tick()
    bd = vfe({'points': torch.from_numpy(g23[tag + '/points']).to(DEV), 'batch_size': 2})
    drv = vfe._pcp_train
    assert isinstance(drv, VFETrain)
    w = drv._weights()
    assert (w['F'], w['fw']) == (c['F'], 16 if c['F'] <= 16 else 32)
    coords = g23[tag + '/voxel_coords']
    assert np.array_equal(bd['voxel_coords'].cpu().numpy(), coords)
    _close(bd['pillar_features'], g23[tag + '/pillar_features'], 2e-5, tag + ' pillar_features (train-mode BN)')
    for li in range(2):
        for k in ('running_mean', 'running_var'):
            _close(getattr(vfe.pfn_layers[li].norm, k), g23['%s/bn/pfn_layers.%d.norm.%s' % (tag, li, k)], 1e-5, '%s %d %s' % (tag, li, k))
    d = c['dpillar']
    P = coords.shape[0]
    R = synth.uniform(d['seed'], d['stream'], P * 64, d['lo'], d['hi']).reshape(P, 64)
    nx, ny = meta['grid_size'][0], meta['grid_size'][1]
    dcanvas = torch.zeros((2, ny, nx, 64), dtype=torch.float32)
    dcanvas[coords[:, 0].astype(np.int64), coords[:, 2].astype(np.int64), coords[:, 3].astype(np.int64)] = torch.from_numpy(R)
    (_name, backward), = bd['_pcp_tape']
    from pcp_amd.train_layers import Act
    backward(Act(dcanvas.to(DEV)))
    tl.flush_batches_tracked()
    params = dict(vfe.named_parameters())
    assert list(params) == c['param_names']
    for name, p in params.items():
        assert tuple(p.grad.shape) == tuple(p.shape)
        _close(p.grad, g23['%s/g/%s' % (tag, name)], 5e-4, '%s d %s' % (tag, name))
    for li in range(2):
        assert int(vfe.pfn_layers[li].norm.num_batches_tracked) == int(g23['%s/bn/pfn_layers.%d.norm.num_batches_tracked' % (tag, li)])


@pytest.mark.parametrize('tag', ['dist', 'one'])
def test_compositions_outside_train_fused_still_refuse_training(tag):
    """WITH_DISTANCE and a one-layer NUM_FILTERS (fixture g16): inference kernels only, and train() says so before touching the device"""
    g = load_golden('g16_pfn_variants.npz')
    v = g['meta']['variants'][tag]
    vfe = _vfe(g['meta'], v['num_raw'], v['use_absolute_xyz'], v['with_distance'], v['vfe_filters'], v['use_norm']).to(DEV).train()
    assert not vfe.train_fused
    with pytest.raises(NotImplementedError, match='inference kernels only'):
        vfe({'points': torch.from_numpy(g[tag + '_points']).to(DEV), 'batch_size': 2})
    wide = _vfe(g['meta'], 27).to(DEV).train()
    with pytest.raises(NotImplementedError, match='at most 26'):
        wide({'points': torch.zeros((8, 28), device=DEV), 'batch_size': 2})


# ---- pointpillar_jr_withmap itself ------------------------------------------------------------------------------------------------------------
# As for nomap (tests/test_gpu_nusc_sc_train.py) there are no reference values at this level: the 60 x 60 mini grid of g20_nusc_mini, its
# withmap weights, its 12-column cloud and seeded 10-column boxes.

@pytest.fixture(scope='module')
def g23m():
    import os
    from pcdet.config import EasyDict, cfg_from_yaml_file
    g = load_golden('g20_nusc_mini.npz')
    meta = dict(g['meta']['cases']['withmap'])
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml = os.path.join(repo, 'practical-collab-perception_amd', 'tools', 'cfgs', 'nuscenes_models', 'pointpillar_jr_withmap.yaml')
    meta['optimization'] = cfg_from_yaml_file(yaml, EasyDict()).OPTIMIZATION
    meta['total_it_each_epoch'] = 5
    return dict(meta=meta, points=g['points_map'], gt_boxes=refs.sc_model_gt(300, meta['pc_range'][3]))


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
    return model, opt, sched


def _model_first_step(g):
    model, opt, sched = _model_and_optimizer(g)
    sched.step(0)
    model.train()
    opt.zero_grad()
    batch = {'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}],
             'gt_boxes': torch.from_numpy(g['gt_boxes']).to(DEV)}
    ret, _tb, _disp = model(batch)
    model.update_global_step()
    ret['loss'].backward()
    return float(ret['loss'].detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, (model, opt)


@pytest.fixture(scope='module')
def model_fp32_step(g23m):
    return _model_first_step(g23m)


def test_withmap_train_step_repeats_bit_for_bit(g23m, model_fp32_step):
    la, ga, (model, _opt) = model_fp32_step
    assert g23m['points'].shape[1] == 13 and model.vfe.num_raw_point_features == 10 and model.vfe.train_fused and not model.vfe.fused
    lb, gb, _ = _model_first_step(g23m)
    assert np.isfinite(la) and la == lb and set(ga) == set(gb) == set(n for n, p in model.named_parameters() if p.requires_grad)
    vfe_names = [n for n in ga if n.startswith('vfe.')]
    assert len(vfe_names) == 6 and tuple(ga['vfe.pfn_layers.0.linear.weight'].shape) == (32, 16)
    assert all(torch.isfinite(ga[n]).all() and float(ga[n].abs().max()) > 0 for n in vfe_names)
    assert not [n for n in ga if not torch.equal(ga[n], gb[n])]


def test_withmap_bf16_loop_iteration_tracks_the_fp32_loss(g23m, model_fp32_step, monkeypatch):
    monkeypatch.setenv('PCP_CONV_ALGO', 'bf16')
    l16, g16, _ = _model_first_step(g23m)
    l32 = model_fp32_step[0]
    print('bf16 loop loss %.6f, fp32 %.6f' % (l16, l32))
    assert np.isfinite(l16) and abs(l16 - l32) <= 1e-2 * abs(l32), (l16, l32)
    assert all(torch.isfinite(v).all() for v in g16.values())


def test_withmap_eval_after_a_train_step_uses_the_stepped_weights(g23m):
    """eval goes through _forward_layers, whose per-layer packed weights the training forward dropped (invalidate_packed): after one
    optimizer step eval() gives the bits of a fresh model loaded from the stepped state_dict()"""
    from pcdet.models import build_network_from_meta
    g = g23m
    st0 = synth.fill_state_dict(g['meta']['state_shapes'], scheme=g['meta']['weight_scheme'])

    def eval_map(m):
        m.eval()
        batch = {'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}]}
        with torch.no_grad():
            m(batch)
        return batch['pillar_features'].clone(), batch['spatial_features_2d'].clone()
    model, opt, sched = _model_and_optimizer(g)
    before = eval_map(model)                                    # packs the layer-wise weights of the UNSTEPPED parameters first
    sched.step(0)
    model.train()
    opt.zero_grad()
    ret, _tb, _disp = model({'points': torch.from_numpy(g['points']).to(DEV), 'batch_size': 2, 'metadata': [{}, {}],
                             'gt_boxes': torch.from_numpy(g['gt_boxes']).to(DEV)})
    model.update_global_step()
    ret['loss'].backward()
    opt.step()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    w0 = 'vfe.pfn_layers.0.linear.weight'
    assert not torch.equal(sd[w0].cpu(), torch.from_numpy(st0[w0]))
    assert all(int(sd['vfe.pfn_layers.%d.norm.num_batches_tracked' % i]) == int(st0['vfe.pfn_layers.%d.norm.num_batches_tracked' % i]) + 1
               for i in range(2))
    got = eval_map(model)
    fresh = build_network_from_meta(g['meta'])
    fresh.load_state_dict(sd)
    want = eval_map(fresh.to(DEV))
    assert not torch.equal(got[0], before[0])
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)
