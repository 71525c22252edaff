"""The device-count forms of the SECOND front end and sparse backbone (include/pcp_hip.h, `_dev`; MODEL.VFE / BACKBONE_3D.DEVICE_COUNTS).

The oracle throughout is the host-count path on the same inputs, itself pinned on float64 restatements by tests/test_gpu_spconv.py: rows
below the count must have its bits, rows at or past the count must keep the sentinel the output was filled with, and the count on the device
must equal the host read.  Inputs behind the count are poisoned (NaN features, coordinates far outside the grid)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(REPO, 'practical-collab-perception_amd')
for p in (os.path.join(REPO, 'tests'), PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import spconv_refs as sr  # noqa: E402
from pcp_amd import ops, synth  # noqa: E402
from pcp_amd import lib as _lib  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 1003)
SHAPE4 = (2, 9, 24, 28)                                   # (B, D, H, W): 12 096 sites
SENT_I, SENT_F = -7, -12345.0
FAR = 0x3fffffff
GUARD = 64
GEOMS = {'s2': ((3, 3, 3), (2, 2, 2), (1, 1, 1)), 'down': ((3, 1, 1), (2, 1, 1), (0, 0, 0))}
_p, _s = ops._p, ops._stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device='cuda')


def _c3(v):
    return (ctypes.c_int32 * 3)(*v)


def _sites(n, seed):
    rng = np.random.default_rng(seed)
    total = int(np.prod(SHAPE4))
    lin = rng.choice(total, size=n, replace=False)
    rng.shuffle(lin)                                       # not in linear order: the table carries a perm
    B, D, H, W = SHAPE4
    return np.stack([lin // (D * H * W), lin // (H * W) % D, lin // W % H, lin % W], 1).astype(np.int32)


def _padded_coords(coords, cap):
    buf = torch.full((cap + GUARD, 4), FAR, dtype=torch.int32, device='cuda')
    buf[:len(coords)] = torch.from_numpy(coords).cuda()
    return buf


def _check(st, what):
    assert st == 0, (what, st)


@functools.lru_cache(maxsize=None)
def tables(n, capmode):
    """both forms of table -> subm -> strided (two geometries) over the same n sites; everything stays on the device"""
    L = _lib.load()
    coords = _sites(n, 100 + n)
    cap = n + 37 if capmode == 'plus37' else max(n, 1)
    out = {'n': n, 'cap': cap, 'coords': coords}
    # ---- host-count form
    hc = torch.from_numpy(coords).cuda() if n else torch.zeros((0, 4), dtype=torch.int32, device='cuda')
    ht = ops.spconv_table(hc, SHAPE4[0], SHAPE4[1:], check_input=True)
    out['h_perm'] = ht.perm[:n].clone()
    out['h_subm'] = ops.spconv_build_subm(hc, ht)
    # ---- device-count form
    dcoords = _padded_coords(coords, cap)
    n_dev = _i32([n])
    mem = torch.empty_like(ht.mem)
    perm = torch.full((cap + GUARD,), SENT_I, dtype=torch.int32, device='cuda')
    counters = torch.full((4,), SENT_I, dtype=torch.int32, device='cuda')
    _check(L.pcp_spconv_table_build_dev(_p(dcoords), _p(n_dev), cap, *SHAPE4, _p(mem), mem.numel(), _p(perm), _p(counters), _s()), 'table')
    nbr = torch.full((27 * cap + GUARD,), SENT_I, dtype=torch.int32, device='cuda')
    _check(L.pcp_spconv_build_subm_dev(_p(dcoords), _p(n_dev), cap, *SHAPE4, _p(mem), mem.numel(), _p(perm), _p(nbr), _s()), 'subm')
    out.update(d_coords=dcoords, n_dev=n_dev, d_mem=mem, d_perm=perm, d_counters=counters, d_subm=nbr)
    for name, (k, s, p) in GEOMS.items():
        hoc, hnbr, hot = ops.spconv_build_strided(hc, ht, k, s, p)
        n_out = int(hoc.shape[0])
        osp = ops.spconv_out_shape(SHAPE4[1:], k, s, p)
        bound = ops.spconv_strided_bound(cap, k, s, (SHAPE4[0],) + osp)
        assert n_out <= bound
        cap_out = n_out + 37 if capmode == 'plus37' else bound
        omem = torch.empty_like(hot.mem)
        cnt = torch.full((4,), SENT_I, dtype=torch.int32, device='cuda')
        err = _i32([0, 0, 0, 0])
        _check(L.pcp_spconv_strided_sites_dev(_p(dcoords), _p(n_dev), cap, *SHAPE4, _c3(k), _c3(s), _c3(p), _p(omem), omem.numel(), cap_out, _p(cnt),
                                              _p(err), 1 << 3, _s()), 'sites')
        oc = torch.full((cap_out + GUARD, 4), SENT_I, dtype=torch.int32, device='cuda')
        K = k[0] * k[1] * k[2]
        onbr = torch.full((K * cap_out + GUARD,), SENT_I, dtype=torch.int32, device='cuda')
        _check(L.pcp_spconv_build_strided_dev(*SHAPE4, _p(mem), mem.numel(), _p(perm), cap, _c3(k), _c3(s), _c3(p), _p(omem), omem.numel(), _p(cnt),
                                              cap_out, _p(oc), _p(onbr), _s()), 'strided')
        out[name] = dict(h_oc=hoc, h_nbr=hnbr, n_out=n_out, cap_out=cap_out, d_oc=oc, d_nbr=onbr, d_cnt=cnt, d_err=err, K=K, d_mem=omem, osp=osp)
    torch.cuda.synchronize()
    return out


def _rows_equal(dev_flat, K, cap, host, n, what):
    """a (K, cap) table stored flat with a guard tail against the host form's (K, n)"""
    body = dev_flat[:K * cap].view(K, cap)
    assert torch.equal(body[:, :n], host), what
    assert bool((body[:, n:] == SENT_I).all()) and bool((dev_flat[K * cap:] == SENT_I).all()), what + ': written at or past the count'


@pytest.mark.parametrize('capmode', ['plus37', 'bound'])
@pytest.mark.parametrize('n', COUNTS)
def test_tables_bit_for_bit(n, capmode):
    t = tables(n, capmode)
    cap = t['cap']
    assert int(t['d_counters'][0]) == n                                                  # the device count is the host read
    assert torch.equal(t['d_perm'][:n], t['h_perm']) and bool((t['d_perm'][n:] == SENT_I).all())
    _rows_equal(t['d_subm'], 27, cap, t['h_subm'], n, 'subm nbr')
    for name in GEOMS:
        g = t[name]
        n_out, cap_out = g['n_out'], g['cap_out']
        assert g['d_cnt'][:3].tolist() == [n_out, 0, n_out] and int(g['d_err'][0]) == 0, name
        assert torch.equal(g['d_oc'][:n_out], g['h_oc']) and bool((g['d_oc'][n_out:] == SENT_I).all()), name
        _rows_equal(g['d_nbr'], g['K'], cap_out, g['h_nbr'], n_out, name + ' nbr')


def _conv_both(feat_rows, cin, nbr_host, nbr_dev_flat, K, n_out, cap_out, n_dev_out, cout, res, relu, seed):
    """host-count conv on exact-shape inputs against the device-count conv on poisoned capacity-sized ones"""
    L = _lib.load()
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn((feat_rows, cin), generator=g).cuda()
    w = ops.spconv_pack_weight((torch.randn((cout, K, 1, 1, cin), generator=g) * 0.2).cuda())
    bias = torch.randn((cout,), generator=g).cuda()
    residual = torch.randn((n_out, cout), generator=g).cuda() if res else None
    want = ops.spconv3d(feats, nbr_host, w, bias, residual=residual, relu=relu)
    fpad = torch.full((feat_rows + 37, cin), float('nan'), device='cuda')
    fpad[:feat_rows] = feats
    rpad = None
    if res:
        rpad = torch.full((cap_out, cout), float('nan'), device='cuda')
        rpad[:n_out] = residual
    out = torch.full((cap_out + GUARD, cout), SENT_F, device='cuda')
    ld_in = cin
    _check(L.pcp_spconv3d_dev(_p(fpad), feat_rows + 37, cin, ld_in, _p(nbr_dev_flat), cap_out, K, _p(n_dev_out), cap_out, _p(w), _p(bias), _p(rpad),
                              1 if relu else 0, cout, _p(out), _s()), 'conv')
    assert torch.equal(out[:n_out].view(torch.int32), want.view(torch.int32))
    assert bool((out[n_out:] == SENT_F).all()), 'conv wrote at or past the count'


# every (cin, cout) of the header's list, plus the raw-width first layer (5 and 11 columns -> 16)
PAIRS = [(5, 16), (11, 16)] + [p for p in ops.SPCONV_CHANNEL_PAIRS]


@pytest.mark.parametrize('res_relu', [(False, False), (True, True)])
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: '%dto%d' % p)
def test_conv_bit_for_bit(pair, res_relu):
    cin, cout = pair
    res, relu = res_relu
    for capmode in ('plus37', 'bound'):
        for n in COUNTS:
            t = tables(n, capmode)
            # the 27-offset submanifold geometry
            _conv_both(n, cin, t['h_subm'], t['d_subm'], 27, n, t['cap'], t['n_dev'], cout, res, relu, seed=n + cin)
            # the 27-offset strided geometry (rows out != rows in) and the 3-offset (3, 1, 1) layer
            for name in GEOMS:
                g = t[name]
                _conv_both(n, cin, g['h_nbr'], g['d_nbr'], g['K'], g['n_out'], g['cap_out'], g['d_cnt'][0:1], cout, res, relu, seed=n + cout)


VFE_RANGE, VFE_VOXEL, VFE_GRID = [0.0, 0.0, 0.0, 5.6, 4.8, 4.0], [0.1, 0.1, 0.1], [56, 48, 40]


def _cloud(n, batch, cols, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 1 + cols), np.float32)
    pts[:, 0] = np.sort(rng.integers(0, batch, n))
    pts[:, 1:4] = rng.uniform(-0.2, 1.0, (n, 3)) * np.asarray(VFE_RANGE[3:], np.float32)      # some rows outside the range
    pts[:, 4:] = rng.normal(size=(n, cols - 3))
    return pts


@pytest.mark.parametrize('cols', [5, 11])
@pytest.mark.parametrize('n', COUNTS)
def test_mean_vfe_features_bit_for_bit(n, cols):
    L = _lib.load()
    B = 2
    pts = torch.from_numpy(_cloud(n, B, cols, 7 + n)).cuda()
    grid = ops.make_grid(VFE_RANGE, VFE_VOXEL, VFE_GRID, B)
    want_f, want_c, M = ops.mean_vfe(pts, grid, cols, nz=VFE_GRID[2])
    need = L.pcp_mean_vfe_workspace_bytes(ctypes.byref(grid), n)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    coords = torch.full((max(n, 1) + GUARD, 4), SENT_I, dtype=torch.int32, device='cuda')
    status = torch.full((ops.DEV_STATUS_WORDS,), SENT_I, dtype=torch.int32, device='cuda')
    feats = torch.full((n + 37, cols), SENT_F, device='cuda')
    _check(L.pcp_mean_vfe(_p(pts), n, 1 + cols, ctypes.byref(grid), VFE_GRID[2], _p(ws), ws.numel(), _p(coords), _p(status), _s()), 'mean_vfe')
    _check(L.pcp_mean_vfe_features_dev(_p(pts), n, 1 + cols, cols, ctypes.byref(grid), VFE_GRID[2], _p(ws), ws.numel(), _p(status), n, _p(feats),
                                       _s()), 'features_dev')
    assert status[:2].tolist() == [M, 0]
    assert torch.equal(feats[:M].view(torch.int32), want_f.view(torch.int32)) and bool((feats[M:] == SENT_F).all())
    assert torch.equal(coords[:M], want_c)
    if n > 100:
        assert 100 < M < n


# ---- the chain without a read ------------------------------------------------------------------------------------------------------------------

class _ReadCensus:
    """counts the device-to-host reads that start inside pcp_amd.ops: Tensor.cpu / .item / .tolist / .numpy wrapped for the forward's duration"""
    NAMES = ('cpu', 'item', 'tolist', 'numpy')

    def __enter__(self):
        self.calls, self._orig = [], {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self._orig[name] = orig

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda and sys._getframe(1).f_globals.get('__name__', '').startswith('pcp_amd.'):
                    self.calls.append(_name)
                return _orig(t, *a, **kw)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self._orig.items():
            setattr(torch.Tensor, name, orig)


def _front_modules(device_counts, cols=5):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.map_to_bev import HeightCompression
    from pcdet.models.backbones_3d import VoxelResBackBone8x
    from pcdet.models.backbones_3d.vfe import DynamicMeanVFE
    extra = {'DEVICE_COUNTS': True} if device_counts else {}
    vfe = DynamicMeanVFE(EasyDict(dict(NAME='DynMeanVFE', **extra)), num_point_features=cols, voxel_size=VFE_VOXEL, grid_size=VFE_GRID,
                         point_cloud_range=VFE_RANGE)
    bb = VoxelResBackBone8x(EasyDict(dict(NAME='VoxelResBackBone8x', **extra)), input_channels=cols, grid_size=np.asarray(VFE_GRID))
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in bb.state_dict().items()})
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    hc = HeightCompression(EasyDict({'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256}))
    return vfe.eval(), bb.cuda().eval(), hc


def test_chain_without_a_read():
    """mean VFE -> table -> subm -> strided -> conv (all 21) -> dense on sr.SECOND_GRID, B = 2: bit-equal maps, no read inside pcp_amd.ops"""
    assert tuple(VFE_GRID[::-1]) == sr.SECOND_GRID
    pts = torch.from_numpy(_cloud(6000, 2, 5, 3)).cuda()
    outs, reads, launches = {}, {}, {}
    for dev in (False, True):
        vfe, bb, hc = _front_modules(dev)
        for _ in range(2):                                  # the second forward reuses the replica's buffers
            batch = {'points': pts, 'batch_size': 2}
            with torch.no_grad(), _ReadCensus() as census:
                batch = hc(bb(vfe(batch)))
            torch.cuda.synchronize()
        outs[dev], reads[dev] = batch, list(census.calls)
    assert len(reads[False]) == 5, reads[False]             # the census sees the host-count form's five reads
    assert reads[True] == [], reads[True]
    a, b = outs[False], outs[True]
    M = int(a['voxel_coords'].shape[0])
    assert M > 1000 and int(b['_pcp_voxel_count'][0]) == M and b['voxel_coords'].shape[0] == 6000
    assert torch.equal(b['voxel_coords'][:M], a['voxel_coords']) and torch.equal(b['voxel_features'][:M], a['voxel_features'])
    for key in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'):
        h, d = a['multi_scale_3d_features'][key], b['multi_scale_3d_features'][key]
        n = int(h.indices.shape[0])
        assert int(d.n_dev[0]) == n and d.capacity >= n and torch.equal(d.indices[:n], h.indices), key
        assert torch.equal(d.features[:n].view(torch.int32), h.features.view(torch.int32)), key
    assert a['spatial_features'].shape == (2, 256, 6, 7) and float(a['spatial_features'].abs().max()) > 0
    assert torch.equal(b['spatial_features'].view(torch.int32), a['spatial_features'].view(torch.int32))
    assert b['_pcp_dev_status'].tolist()[1] == 0 and b['_pcp_dev_status'].tolist()[ops.DEV_STATUS_OVERFLOW] == 0


# ---- whole models ------------------------------------------------------------------------------------------------------------------------------

MINI_RANGE = [-6.4, -6.4, -8.0, 6.4, 6.4, 0.0]            # 128 x 128 x 40 voxels of (0.1, 0.1, 0.2)
YAMLS = {'ego': 'cfgs/v2x_sim_models/v2x_second_ego.yaml', 'rsu': 'cfgs/v2x_sim_models/v2x_second_rsu.yaml'}


def _mini_model(which, device_counts, tmp_path, vfe_only=False, hip_train=False):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import SyntheticV2XDataset
    from pcdet.models import build_network
    cwd = os.getcwd()
    os.chdir(os.path.join(PKG, 'tools'))
    try:
        cfg = cfg_from_yaml_file(YAMLS[which], EasyDict())
    finally:
        os.chdir(cwd)
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = list(MINI_RANGE)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=4000, NUM_FRAMES=3, DISTRIBUTION='uniform')
    if which == 'rsu':
        cfg.MODEL.CORRECTOR.DATABASE_EXCHANGE_DATA = str(tmp_path)
        cfg.MODEL.DENSE_HEAD.DATABASE_EXCHANGE_DATA = str(tmp_path)
    if device_counts:
        cfg.MODEL.VFE.DEVICE_COUNTS = True
        cfg.MODEL.BACKBONE_3D.DEVICE_COUNTS = not vfe_only
    if hip_train:
        cfg.MODEL.VFE.HIP_TRAIN = True
        cfg.MODEL.BACKBONE_3D.HIP_TRAIN = True
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval(), ds


def _batch(ds, idx):
    from pcdet.models import load_data_to_gpu
    batch = ds.collate_batch([ds[i] for i in idx])
    load_data_to_gpu(batch)
    return batch


def _sets(pred):
    return [(p['pred_boxes'].cpu().numpy(), p['pred_scores'].cpu().numpy(), p['pred_labels'].cpu().numpy()) for p in pred]


def _preds(model, ds, idx):
    batch = _batch(ds, idx)
    with torch.no_grad():
        pred, _ = model(batch)
    torch.cuda.synchronize()
    return _sets(pred), batch


def _same(a, b, what=''):
    assert len(a) == len(b), what
    for fa, fb in zip(a, b):
        for u, v in zip(fa, fb):
            assert u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), what


@pytest.mark.parametrize('which', ['ego', 'rsu'])
def test_whole_model_with_the_switch(which, tmp_path):
    from pcdet.models.pipelined import PipelinedDetector
    host, ds = _mini_model(which, False, tmp_path)
    dev, _ = _mini_model(which, True, tmp_path)
    assert not PipelinedDetector.supports(host) and PipelinedDetector.supports(dev)
    idx_sets = [[0, 1, 2], [1, 2], [2, 0], [1]]
    want = [_preds(host, ds, idx)[0] for idx in idx_sets]
    assert sum(f[0].shape[0] for w in want for f in w) > 0
    for idx, w in zip(idx_sets, want):
        _same(_preds(dev, ds, idx)[0], w, 'model(batch) %s' % idx)
    _same(_preds(dev, ds, idx_sets[0])[0], want[0], 'repeat')
    for i in range(3):                                      # a frame alone has the bits it has inside a batch
        _same(_preds(dev, ds, [i])[0], [want[0][i]], 'frame %d alone' % i)
    pipe = PipelinedDetector(dev, replicas=2)
    assert len(pipe.models) == 2
    got = []
    for idx in idx_sets:
        b = _batch(ds, idx)
        prev = pipe.submit(b['points'], b['batch_size'], b.get('metadata', None), extra=b)
        if prev is not None:
            got.append(_sets(prev))
    got.append(_sets(pipe.flush()))
    torch.cuda.synchronize()
    for idx, g, w in zip(idx_sets, got, want):
        _same(g, w, 'pipelined %s' % idx)


def test_build_time_refusals(tmp_path):
    with pytest.raises(ValueError, match='DEVICE_COUNTS'):
        _mini_model('ego', True, tmp_path, vfe_only=True)
    with pytest.raises(NotImplementedError, match='HIP_TRAIN'):
        _mini_model('ego', True, tmp_path, hip_train=True)


def test_tools_test_py_fast_pipelines_the_switched_model():
    tools = os.path.join(PKG, 'tools')
    cmd = [sys.executable, 'test.py', '--cfg_file', YAMLS['ego'], '--batch_size', '2', '--fast',
           '--set', 'DATA_CONFIG.POINT_CLOUD_RANGE', ','.join(str(v) for v in MINI_RANGE), 'DATA_CONFIG.SYNTHETIC.POINTS_PER_AGENT', '3000',
           'DATA_CONFIG.SYNTHETIC.NUM_FRAMES', '3', 'MODEL.VFE.DEVICE_COUNTS', 'True', 'MODEL.BACKBONE_3D.DEVICE_COUNTS', 'True']
    r = subprocess.run(cmd, cwd=tools, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    out = r.stdout + r.stderr
    assert 'pipelined over 2 model replicas' in out and 'over 3 frames' in out, out[-1500:]


# ---- overflow and deferred errors ----------------------------------------------------------------------------------------------------------------

def test_row_capacity_one_short_raises_at_the_final_read(tmp_path):
    """every write of the build and conv kernels is guarded by min(*n_dev, capacity) (csrc/spconv3d.hip: dev_rows; the scan clamps the count
    it leaves, k_sp_table_coords tests rank < count, the nbr kernels and k_spconv3d test row < count): a level one row short drops its last
    row, sets its bit, and the final read names it"""
    host, ds = _mini_model('ego', False, tmp_path)
    _w, hb = _preds(host, ds, [0, 1, 2])
    rows = [int(hb['multi_scale_3d_features'][k].indices.shape[0]) for k in ('x_conv2', 'x_conv3', 'x_conv4')]
    dev, _ = _mini_model('ego', True, tmp_path)
    dev.backbone_3d.row_capacity = [None, None, rows[1] - 1, None, None]
    with pytest.raises(RuntimeError, match=r'level 2 \(spconv3, ROW_CAPACITY %d\)' % (rows[1] - 1)):
        _preds(dev, ds, [0, 1, 2])
    torch.cuda.synchronize()
    dev.backbone_3d.row_capacity = [None, rows[0], rows[1], rows[2], None]                # exactly enough: no error, same sets
    _same(_preds(dev, ds, [0, 1, 2])[0], _w, 'exact capacities')


def test_clamped_build_writes_nothing_past_the_capacity():
    L = _lib.load()
    t = tables(1003, 'plus37')
    k, s, p = GEOMS['s2']
    g = t['s2']
    cap_out = g['n_out'] - 1
    cnt = torch.full((4,), SENT_I, dtype=torch.int32, device='cuda')
    err = _i32([0, 0, 0, 0])
    omem = torch.empty_like(g['d_mem'])
    _check(L.pcp_spconv_strided_sites_dev(_p(t['d_coords']), _p(t['n_dev']), t['cap'], *SHAPE4, _c3(k), _c3(s), _c3(p), _p(omem), omem.numel(), cap_out,
                                          _p(cnt), _p(err), 1 << 3, _s()), 'sites')
    oc = torch.full((cap_out + GUARD, 4), SENT_I, dtype=torch.int32, device='cuda')
    onbr = torch.full((27 * cap_out + GUARD,), SENT_I, dtype=torch.int32, device='cuda')
    _check(L.pcp_spconv_build_strided_dev(*SHAPE4, _p(t['d_mem']), t['d_mem'].numel(), _p(t['d_perm']), t['cap'], _c3(k), _c3(s), _c3(p), _p(omem),
                                          omem.numel(), _p(cnt), cap_out, _p(oc), _p(onbr), _s()), 'strided')
    assert cnt[:3].tolist() == [cap_out, 0, g['n_out']] and int(err[0]) == 1 << 3
    assert torch.equal(oc[:cap_out], g['h_oc'][:cap_out]) and bool((oc[cap_out:] == SENT_I).all())          # the tail is what is dropped
    assert torch.equal(onbr[:27 * cap_out].view(27, cap_out), g['h_nbr'][:, :cap_out]) and bool((onbr[27 * cap_out:] == SENT_I).all())
    # the next level over the clamped set: its lookups treat the dropped row as absent
    k2, s2, p2 = GEOMS['down']
    shape_o = (SHAPE4[0],) + tuple(g['osp'])
    osp2 = ops.spconv_out_shape(g['osp'], k2, s2, p2)
    mem2 = torch.empty(L.pcp_spconv_table_bytes(SHAPE4[0], *osp2), dtype=torch.uint8, device='cuda')
    cnt2 = torch.full((4,), SENT_I, dtype=torch.int32, device='cuda')
    cap2 = ops.spconv_strided_bound(cap_out, k2, s2, (SHAPE4[0],) + osp2)
    _check(L.pcp_spconv_strided_sites_dev(_p(oc), _p(cnt), cap_out, *shape_o, _c3(k2), _c3(s2), _c3(p2), _p(mem2), mem2.numel(), cap2, _p(cnt2),
                                          _p(err), 1 << 4, _s()), 'sites 2')
    nbr2 = torch.full((3 * cap2 + GUARD,), SENT_I, dtype=torch.int32, device='cuda')
    oc2 = torch.full((cap2 + GUARD, 4), SENT_I, dtype=torch.int32, device='cuda')
    _check(L.pcp_spconv_build_strided_dev(*shape_o, _p(omem), omem.numel(), None, cap_out, _c3(k2), _c3(s2), _c3(p2), _p(mem2), mem2.numel(),
                                          _p(cnt2), cap2, _p(oc2), _p(nbr2), _s()), 'strided 2')
    n2 = int(cnt2[0])
    body = nbr2[:3 * cap2].view(3, cap2)[:, :n2]
    assert n2 > 0 and int(body.max()) < cap_out and int(err[0]) == 1 << 3


def test_frames_out_of_order_raise_the_deferred_value_error(tmp_path):
    host, ds = _mini_model('ego', False, tmp_path)
    dev, _ = _mini_model('ego', True, tmp_path)
    for model in (host, dev):
        batch = _batch(ds, [0, 1])
        pts = batch['points']
        batch['points'] = torch.cat([pts[pts[:, 0] == 1], pts[pts[:, 0] == 0]]).contiguous()
        with pytest.raises(ValueError, match='ascending frame index'):
            with torch.no_grad():
                model(batch)
        torch.cuda.synchronize()


def test_exact_bound_on_isolated_voxels():
    """odd coordinates four apart: each voxel reaches 2 x 2 x 2 outputs of the 3 / 2 / pad 1 layer, none shared -- the bound 8 n is met"""
    k, s, p = GEOMS['s2']
    B, D, H, W = SHAPE4
    zz, yy, xx = np.meshgrid(np.arange(1, D - 1, 4), np.arange(1, H - 1, 4), np.arange(1, W - 1, 4), indexing='ij')
    one = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], 1)
    coords = np.concatenate([np.concatenate([np.full((len(one), 1), b), one], 1) for b in range(B)]).astype(np.int32)
    n = len(coords)
    assert n > 64 and len(sr.strided_out_coords(coords, SHAPE4, k, s, p)) == 8 * n
    hc = torch.from_numpy(coords).cuda()
    ht = ops.spconv_table(hc, B, SHAPE4[1:])
    hoc, hnbr, _hot = ops.spconv_build_strided(hc, ht, k, s, p)
    assert hoc.shape[0] == 8 * n
    n_dev = _i32([n])
    status = torch.zeros((ops.DEV_STATUS_WORDS,), dtype=torch.int32, device='cuda')
    dt = ops.spconv_table_dev(hc, n_dev, B, SHAPE4[1:])
    oc, nbr, ot, n_out = ops.spconv_build_strided_dev(hc, dt, n_dev, k, s, p, status=status, level=1)
    assert ot.capacity == 8 * n == int(n_out[0]) and status.tolist() == [0] * ops.DEV_STATUS_WORDS
    assert torch.equal(oc, hoc) and torch.equal(nbr, hnbr)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn((n, 16), generator=g).cuda()
    w = ops.spconv_pack_weight((torch.randn((32, 3, 3, 3, 16), generator=g) * 0.2).cuda())
    bias = torch.randn((32,), generator=g).cuda()
    want = ops.spconv3d(feats, hnbr, w, bias, relu=True)
    got = ops.spconv3d_dev(feats, nbr, n_out, w, bias, relu=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- both forms through ops alone ----------------------------------------------------------------------------------------------------------------

def _poisoned(rows, cap, fill):
    buf = torch.full((cap,) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device='cuda')
    buf[:rows.shape[0]] = rows
    return buf


@pytest.mark.parametrize('n', [0, 1, 17, 65])
def test_both_forms_through_the_ops_wrappers(n):
    """table -> subm -> conv 16 -> 16 -> strided (both geometries) -> conv 32 -> 64 -> dense, residual and ReLU on, through ops.* and ops.*_dev
    only (the bit comparisons above call the `_dev` symbols themselves): rows below the count and the dense maps bit-equal, the device count
    the host's, and a second device-count pass over the same DevBuffers allocates nothing"""
    B, sp = SHAPE4[0], SHAPE4[1:]
    g = torch.Generator().manual_seed(900 + n)

    def rand(*shape):
        return torch.randn(shape, generator=g).cuda()
    coords = torch.from_numpy(_sites(n, 300 + n)).cuda() if n else torch.zeros((0, 4), dtype=torch.int32, device='cuda')
    f16, f32, res16 = rand(n, 16), rand(n, 32), rand(n, 16)
    w16, b16 = ops.spconv_pack_weight(rand(16, 3, 3, 3, 16) * 0.2), rand(16)
    # ---- host counts
    ht = ops.spconv_table(coords, B, sp)
    hsub = ops.spconv_build_subm(coords, ht)
    hc1 = ops.spconv3d(f16, hsub, w16, b16, residual=res16, relu=True)
    hd1 = ops.spconv_dense(hc1, ht)
    host = {}
    for name, (k, s, p) in GEOMS.items():
        oc, nbr, ot = ops.spconv_build_strided(coords, ht, k, s, p)
        w, b, res = ops.spconv_pack_weight(rand(64, *k, 32) * 0.2), rand(64), rand(int(oc.shape[0]), 64)
        out = ops.spconv3d(f32, nbr, w, b, residual=res, relu=True)
        host[name] = dict(oc=oc, nbr=nbr, w=w, b=b, res=res, out=out, dense=ops.spconv_dense(out, ot), shape4=ot.shape4)
    # ---- device counts: capacity-sized inputs, poisoned behind the count; one DevBuffers, two passes
    cap = n + 5
    dcoords, n_dev = _poisoned(coords, cap, FAR), _i32([n])
    df16, df32, dres16 = (_poisoned(t, cap, float('nan')) for t in (f16, f32, res16))
    bufs, held = ops.DevBuffers(), None
    for _pass in range(2):
        status = torch.zeros((ops.DEV_STATUS_WORDS,), dtype=torch.int32, device='cuda')
        dt = ops.spconv_table_dev(dcoords, n_dev, B, sp, bufs=bufs)
        assert dt.capacity == cap and dt.shape4 == ht.shape4 and torch.equal(dt.perm[:n], ht.perm[:n])
        dsub = ops.spconv_build_subm_dev(dcoords, dt, n_dev, bufs=bufs, name='subm0')
        assert tuple(dsub.shape) == (27, cap) and torch.equal(dsub[:, :n], hsub)
        dc1 = ops.spconv3d_dev(df16, dsub, n_dev, w16, b16, residual=dres16, relu=True, bufs=bufs, name='conv1')
        assert tuple(dc1.shape) == (cap, 16) and torch.equal(dc1[:n].view(torch.int32), hc1.view(torch.int32))
        assert torch.equal(ops.spconv_dense(dc1, dt).view(torch.int32), hd1.view(torch.int32))
        for level, (name, (k, s, p)) in enumerate(GEOMS.items(), 1):
            h = host[name]
            n_out = int(h['oc'].shape[0])
            oc, nbr, ot, n_out_dev = ops.spconv_build_strided_dev(dcoords, dt, n_dev, k, s, p, status=status, level=level, bufs=bufs, name=name)
            cap_out = ot.capacity
            assert int(n_out_dev[0]) == n_out and cap_out >= max(n_out, 1) and ot.shape4 == h['shape4'], name
            assert tuple(oc.shape) == (cap_out, 4) and tuple(nbr.shape) == (k[0] * k[1] * k[2], cap_out), name
            assert torch.equal(oc[:n_out], h['oc']) and torch.equal(nbr[:, :n_out], h['nbr']), name
            out = ops.spconv3d_dev(df32, nbr, n_out_dev, h['w'], h['b'], residual=_poisoned(h['res'], cap_out, float('nan')), relu=True, bufs=bufs,
                                   name='conv_' + name)
            assert tuple(out.shape) == (cap_out, 64) and torch.equal(out[:n_out].view(torch.int32), h['out'].view(torch.int32)), name
            assert torch.equal(ops.spconv_dense(out, ot).view(torch.int32), h['dense'].view(torch.int32)), name
        assert status.tolist() == [0] * ops.DEV_STATUS_WORDS
        now = {key: (t.data_ptr(), t.numel()) for key, t in bufs._t.items()}
        assert held is None or now == held, 'the second pass allocated'
        held = now
    assert sorted(held) == sorted(['table0', 'perm0', 'nbr_subm0', 'feat_conv1'] + [pre + name for name in GEOMS
                                                                                    for pre in ('table_', 'coords_', 'nbr_', 'feat_conv_')])
