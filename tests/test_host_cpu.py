"""CPU-side checks (no GPU): the C-ABI library loads and exports every declared symbol, the reference-compatible plugin surface
builds the same parameter tree as the reference (key names + shapes recorded by make_golden.py), BatchNorm folding and
weight packing reproduce the oracle's convolutions, the config API behaves like the reference's, and the product path
refuses to run without CUDA tensors."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pack_eval
from helpers import GOLDEN, load_golden
from pcp_amd import pack, synth

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def test_library_exports_every_symbol_of_the_header():
    from pcp_amd import lib
    L = lib.load()
    header = ''.join(open(os.path.join(REPO, 'include', h)).read() for h in sorted(os.listdir(os.path.join(REPO, 'include'))))
    declared = set(re.findall(r'\b(pcp_[a-z0-9_]+)\s*\(', header))
    assert declared, 'no declarations parsed'
    for name in declared:
        assert hasattr(L, name), 'header declares %s but the library does not export it' % name
    assert declared == set(lib.SYMBOLS.keys()), declared ^ set(lib.SYMBOLS.keys())
    assert L.pcp_abi_version() == 1
    assert L.pcp_status_string(2).decode() == 'workspace too small'


@pytest.mark.parametrize('tag', ['car', 'ego', 'early', 'disco'])
def test_state_dict_keys_and_shapes_equal_the_reference(tag):
    from pcdet.models import build_network_from_meta
    g = load_golden('g1_%s.npz' % tag)
    model = build_network_from_meta(g['meta'])
    mine = {k: list(v.shape) for k, v in model.state_dict().items()}
    ref = g['meta']['state_shapes']
    assert set(mine) == set(ref), sorted(set(mine) ^ set(ref))[:10]
    for k in ref:
        assert mine[k] == ref[k], (k, mine[k], ref[k])
    # loading reference-named weights works through the reference's own entry point semantics
    st = synth.fill_state_dict(ref)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    names = [type(m).__name__ for m in model.module_list]
    assert names[-1] == 'CenterHead' and 'DynamicPillarVFE' in names


def test_product_path_fails_loudly_without_gpu():
    from pcdet.models import build_network_from_meta
    from pcp_amd.lib import PcpError
    g = load_golden('g1_ego.npz')
    model = build_network_from_meta(g['meta']).eval()
    batch = {'points': torch.from_numpy(g['points']), 'batch_size': 2, 'metadata': [{}, {}]}
    with pytest.raises((PcpError, RuntimeError)):
        model(batch)
    # train mode has no CPU path either: the HIP training kernels refuse host tensors
    model.train()
    batch = {'points': torch.from_numpy(g['points']), 'batch_size': 2, 'metadata': [{}, {}], 'gt_boxes': torch.zeros(2, 1, 8)}
    with pytest.raises((PcpError, RuntimeError)):
        model(batch)
    # modules without training kernels say so (HunterJr: inference branch only)
    gc = load_golden('g1_car.npz')
    car = build_network_from_meta(gc['meta']).train()
    with pytest.raises((NotImplementedError, PcpError, RuntimeError)):
        car({'points': torch.from_numpy(gc['points']), 'batch_size': 2, 'metadata': [{}, {}], 'gt_boxes': torch.zeros(2, 1, 8)})


def test_product_never_touches_the_oracle_or_the_reference():
    """the oracle is test infrastructure: nothing under the product package (nor bench.py outside its cpu_baseline leg) may import it,
    and nothing shipped may read /root/reference at run time"""
    import re
    pkg = os.path.join(REPO, 'practical-collab-perception_amd')
    offenders = []
    for root, _dirs, files in os.walk(pkg):
        for f in files:
            if not f.endswith(('.py', '.hip', '.h', '.sh')) and f != 'Makefile':
                continue
            text = open(os.path.join(root, f), errors='ignore').read()
            if re.search(r'^\s*(from|import)\s+oracle\b', text, re.M) or '/root/reference' in text:
                offenders.append(os.path.join(root, f))
    assert offenders == [], offenders
    bench = open(os.path.join(REPO, 'bench.py')).read()
    uses = [m.start() for m in re.finditer(r'from oracle|import oracle', bench)]
    assert len(uses) >= 1
    for u in uses:                                   # every import of the oracle sits inside a top-level cpu_baseline* function
        top = bench.rfind('\ndef ', 0, u)
        assert bench[top + 1:top + 17] == 'def cpu_baseline', bench[top:top + 60]
    assert '/root/reference' not in bench           # (__graft_entry__.build() only probes for it to rebuild oracle/_ref in this container)


def test_bn_folding_and_conv3x3_packing_roundtrip():
    cin, cout = 32, 40
    w = torch.from_numpy(synth.uniform(1, 1, cout * cin * 9, -0.1, 0.1).reshape(cout, cin, 3, 3))
    gamma = torch.from_numpy(synth.uniform(1, 2, cout, 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform(1, 3, cout, -0.1, 0.1))
    mean = torch.from_numpy(synth.uniform(1, 4, cout, -0.1, 0.1))
    var = torch.from_numpy(synth.uniform(1, 5, cout, 0.5, 1.5))
    x = torch.from_numpy(synth.uniform(1, 6, 2 * cin * 10 * 12, -1, 1).reshape(2, cin, 10, 12))
    want = F.batch_norm(F.conv2d(x, w, None, padding=1), mean, var, gamma, beta, False, 0.0, 1e-3)
    wf, bf = pack.fold_bn(w, gamma, beta, mean, var, 1e-3)
    packed, bp, cpad = pack.pack_conv3x3(wf, bf)
    assert packed.shape == (cin // 16, 9, cpad, 16) and cpad == 64 and bp.shape == (64,)
    w_back = pack_eval.unpack_conv3x3(packed, cout, cin)
    got = F.conv2d(x, w_back, bp[:cout], padding=1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert float(packed[:, :, cout:].abs().max()) == 0.0            # padded output channels are zero


def test_winograd4_packing_evaluates_to_the_convolution():
    """F(4x4,3x3) filter transform + [36][cout_pad][cin] layout: the packed form evaluated with the kernel's transform matrices in
    float64 equals the direct convolution (the fp32 rounding of the device path is bounded in tests/test_gpu_ops.py)"""
    cin, cout = 32, 12
    w = torch.from_numpy(synth.uniform(7, 1, cout * cin * 9, -0.1, 0.1).reshape(cout, cin, 3, 3))
    b = torch.from_numpy(synth.uniform(7, 2, cout, -0.2, 0.2))
    x = torch.from_numpy(synth.uniform(7, 3, 2 * cin * 8 * 12, -1, 1).reshape(2, cin, 8, 12))
    packed, bp, cpad = pack.pack_conv3x3_winograd4(w, b)
    assert packed.shape == (36, 128, cin) and cpad == 128 and float(packed[:, cout:].abs().max()) == 0.0
    got = pack_eval.winograd4_reference(x.double(), packed.double(), bp.double(), cout)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=5e-6)      # U is rounded to fp32 once; A^T amplifies by <= 8 x 8


def test_pointwise_packings_match_torch_convs():
    cin, cout = 32, 24
    x = torch.from_numpy(synth.uniform(2, 1, 1 * cin * 6 * 8, -1, 1).reshape(1, cin, 6, 8))
    b = torch.zeros(cout)
    # Conv2d k2 s2: K ordered (tap, cin)
    w = torch.from_numpy(synth.uniform(2, 2, cout * cin * 4, -0.1, 0.1).reshape(cout, cin, 2, 2))
    packed, _, cpad = pack.pack_conv2x2_s2(w, b)
    mat = pack_eval.unpack_plain(packed, cout)                            # (cout, 4*cin)
    xs = torch.stack([x[:, :, ky::2, kx::2] for ky in range(2) for kx in range(2)], 1).reshape(1, 4 * cin, 3, 4)
    got = torch.einsum('nk,bkhw->bnhw', mat, xs)
    np.testing.assert_allclose(got.numpy(), F.conv2d(x, w, None, stride=2).numpy(), rtol=1e-5, atol=1e-5)
    # ConvTranspose2d k2 s2: N ordered (tap, cout_pad)
    wt = torch.from_numpy(synth.uniform(2, 3, cin * cout * 4, -0.1, 0.1).reshape(cin, cout, 2, 2))
    packed, _, cpad = pack.pack_convT2x2_s2(wt, b)
    mat = pack_eval.unpack_plain(packed, 4 * cpad)                        # (4*cpad, cin)
    y = torch.einsum('nk,bkhw->bnhw', mat, x).reshape(1, 2, 2, cpad, 6, 8)[:, :, :, :cout]
    out = torch.zeros(1, cout, 12, 16)
    for ky in range(2):
        for kx in range(2):
            out[:, :, ky::2, kx::2] = y[:, ky, kx]
    np.testing.assert_allclose(out.numpy(), F.conv_transpose2d(x, wt, None, stride=2).numpy(), rtol=1e-5, atol=1e-5)


def test_config_api(tmp_path):
    from pcdet.config import EasyDict, cfg_from_list, cfg_from_yaml_file
    base = tmp_path / 'base.yaml'
    base.write_text('DATASET: X\nPOINT_CLOUD_RANGE: [0, 1, 2, 3, 4, 5]\nNESTED: {A: 1, B: [1, 2]}\n')
    top = tmp_path / 'top.yaml'
    top.write_text('CLASS_NAMES: [car]\nDATA_CONFIG:\n    _BASE_CONFIG_: %s\n    NESTED: {A: 7}\nMODEL: {NAME: CenterPoint, LR: 0.1}\n' % base)
    cfg = cfg_from_yaml_file(str(top), EasyDict())
    assert cfg.DATA_CONFIG.DATASET == 'X' and cfg.DATA_CONFIG.NESTED.A == 7 and cfg.DATA_CONFIG.NESTED.B == [1, 2]
    cfg_from_list(['MODEL.LR', '0.5', 'DATA_CONFIG.NESTED.A', '9'], cfg)
    assert cfg.MODEL.LR == 0.5 and cfg['DATA_CONFIG']['NESTED']['A'] == 9
    with pytest.raises(AssertionError):
        cfg_from_list(['MODEL.MISSING', '1'], cfg)
    with pytest.raises(AssertionError):
        cfg_from_list(['MODEL.NAME', '3'], cfg)                      # type mismatch str vs int


def test_shipped_yaml_configs_build_all_five_models():
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    cfg_dir = os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models')
    expected = {'v2x_pointpillar_basic_car.yaml': ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'HunterJr', 'CenterHead'],
                'v2x_pointpillar_basic_ego.yaml': ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'CenterHead'],
                'v2x_pointpillar_basic_ego_early.yaml': ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'CenterHead'],
                'v2x_pointpillar_disco.yaml': ['BEVMaker', 'BEVMaker', 'BEVMaker', 'DynamicPillarVFE', 'PointPillarScatter',
                                               'BaseBEVBackbone', 'V2XMidFusionDisco', 'CenterHead'],
                'v2x_pointpillar_anchor.yaml': ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'AnchorHeadSingle']}
    for name, mods in expected.items():
        cfg = cfg_from_yaml_file(os.path.join(cfg_dir, name), EasyDict())
        for key in ('BEV_MAKER_RSU', 'BEV_MAKER_CAR', 'BEV_MAKER_EARLY'):
            if cfg.MODEL.get(key, None) is not None:
                cfg.MODEL[key].CKPT = None
        enc = cfg.DATA_CONFIG.POINT_FEATURE_ENCODING
        vs = [p.VOXEL_SIZE for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
        ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(enc.used_feature_list))
        model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
        assert [type(m).__name__ for m in model.module_list] == mods, name
        assert list(ds.grid_size) == [512, 512, 1]
        if name == 'v2x_pointpillar_anchor.yaml':
            assert type(model).__name__ == 'PointPillar' and model.dense_head.num_anchors_per_location == 2
            assert tuple(model.dense_head.anchors[0].shape) == (1, 128, 128, 1, 2, 7)
            assert sorted(k for k in model.state_dict() if k.startswith('dense_head.')) == [
                'dense_head.conv_box.bias', 'dense_head.conv_box.weight', 'dense_head.conv_cls.bias', 'dense_head.conv_cls.weight',
                'dense_head.conv_dir_cls.bias', 'dense_head.conv_dir_cls.weight']


@pytest.mark.parametrize('yaml_name,golden', [('v2x_pointpillar_basic_car.yaml', 'g1_car.npz'), ('v2x_pointpillar_basic_rsu.yaml', 'g1_rsu.npz'),
                                              ('v2x_pointpillar_basic_ego.yaml', 'g1_ego.npz'), ('v2x_pointpillar_basic_ego_early.yaml', 'g1_early.npz'),
                                              ('v2x_pointpillar_disco.yaml', 'g1_disco.npz')])
def test_shipped_yaml_state_dicts_equal_the_references(yaml_name, golden):
    """every shipped YAML builds a model whose state-dict keys and shapes are EXACTLY those of the reference model built from the
    reference's YAML of the same name (recorded as data in the golden fixtures): reference checkpoints load with strict=True"""
    from helpers import GOLDEN, load_golden
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.models import DatasetInfo, build_network
    cfg = cfg_from_yaml_file(os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models', yaml_name), EasyDict())
    for key in ('BEV_MAKER_RSU', 'BEV_MAKER_CAR', 'BEV_MAKER_EARLY'):
        if cfg.MODEL.get(key, None) is not None:
            cfg.MODEL[key].CKPT = None
    enc = cfg.DATA_CONFIG.POINT_FEATURE_ENCODING
    vs = [p.VOXEL_SIZE for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(enc.used_feature_list))
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    ref = {k: tuple(v) for k, v in load_golden(golden)['meta']['state_shapes'].items()}
    assert sorted(mine) == sorted(ref), sorted(set(mine) ^ set(ref))[:10]
    assert all(mine[k] == ref[k] for k in ref), [k for k in ref if mine[k] != ref[k]][:10]


@pytest.mark.parametrize('yaml_name,golden,opt_golden', [
    ('v2x_pointpillar_basic_car.yaml', 'g1_car.npz', 'g12_hunter_train.npz'), ('v2x_pointpillar_basic_rsu.yaml', 'g1_rsu.npz', None),
    ('v2x_pointpillar_basic_ego.yaml', 'g1_ego.npz', 'g7b_train_ego.npz'), ('v2x_pointpillar_basic_ego_early.yaml', 'g1_early.npz', None),
    ('v2x_pointpillar_disco.yaml', 'g1_disco.npz', 'g7_train.npz')])
def test_shipped_yaml_sections_equal_the_references(yaml_name, golden, opt_golden):
    """the resolved MODEL (and OPTIMIZATION) section of every shipped YAML against the reference's resolved section of the YAML of the same
    name (stored as data with the golden fixtures): equal key by key except the build's own include keys, keys the build adds with the
    reference's default, and the overrides the fixture generator applied (temp checkpoints, mini-geometry range, lowered score threshold)"""
    from helpers import GOLDEN, load_golden
    from pcdet.config import EasyDict, cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models', yaml_name), EasyDict())

    def plain(d):
        if isinstance(d, dict):
            return {k: plain(v) for k, v in d.items()}
        return [plain(v) for v in d] if isinstance(d, (list, tuple)) else d

    def diff(a, b, path=''):
        if isinstance(a, dict) and isinstance(b, dict):
            out = []
            for k in sorted(set(a) | set(b)):
                out += [(path + '/' + k, a.get(k, '<absent>'), b.get(k, '<absent>'))] if (k not in a or k not in b) else diff(a[k], b[k], path + '/' + k)
            return out
        if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
            return [d for i, (x, y) in enumerate(zip(a, b)) for d in diff(x, y, '%s[%d]' % (path, i))]
        same = a == b or (isinstance(a, (int, float)) and isinstance(b, (int, float)) and abs(a - b) < 1e-12)
        return [] if same else [(path, a, b)]
    allowed = ('_BASE_CONFIG_', '/CKPT', '/DEBUG', 'GENERATING_EXCHANGE_DATA', 'DATABASE_EXCHANGE_DATA', 'PC_RANGE_MIN', 'BACKBONE_2D/BACKBONE_2D',
               'POST_PROCESSING/SCORE_THRESH')
    left = [d for d in diff(plain(cfg.MODEL), load_golden(golden)['meta']['model']) if not any(a in d[0] for a in allowed)]
    assert not left, left
    assert cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH == 0.1                       # the reference's value (fixtures lower it to 0.02)
    if opt_golden is not None:
        left = [d for d in diff(plain(cfg.OPTIMIZATION), load_golden(opt_golden)['meta']['optimization']) if '_BASE_CONFIG_' not in d[0]]
        assert not left, left


def test_training_dataset_and_onecycle_schedule():
    """synthetic training items carry zero-padded gt_boxes (collate_batch contract, dataset.py:260-266); the one-cycle schedule
    reproduces the lr / beta1 values the reference's scheduler produced for the golden run"""
    import sys
    sys.path.insert(0, os.path.join(REPO, 'practical-collab-perception_amd', 'tools'))
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    from train_utils.optimization import OneCycle
    cfg = cfg_from_yaml_file(os.path.join(REPO, 'practical-collab-perception_amd', 'tools', 'cfgs', 'v2x_sim_models', 'v2x_pointpillar_disco.yaml'),
                             EasyDict())
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=200, NUM_FRAMES=5)
    ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, 3, False, training=True)
    batch = next(iter(loader))
    gt = batch['gt_boxes']
    assert gt.shape[0] == 3 and gt.shape[2] == 8 and batch['points'].shape[1] == 7
    assert (gt[..., 7] >= 0).all() and (gt[..., 7] <= len(cfg.CLASS_NAMES)).all()
    lens = [(gt[b, :, 7] > 0).sum() for b in range(3)]
    assert len(set(lens)) > 1 and (gt[np.argmin(lens), min(lens):] == 0).all()       # ragged frames, zero padding
    g = load_golden('g7_train.npz')
    oc = g['meta']['optimization']

    class Opt:
        lr = mom = 0.0
    sched = OneCycle(Opt, g['meta']['total_it_each_epoch'] * oc['NUM_EPOCHS'], oc['LR'], oc['MOMS'], oc['DIV_FACTOR'], oc['PCT_START'])
    for it in range(2):
        sched.step(it)
        assert abs(Opt.lr - float(g['it%d_lr' % it])) < 1e-15 and abs(Opt.mom - float(g['it%d_mom' % it])) < 1e-15


def test_winograd_ws_packing_holds_the_same_transformed_weights():
    """pack_conv3x3_winograd_ws is a re-ordering of the same U = G g G^T the fused kernel's packing holds (layout check on the CPU; the
    packed form evaluated in plain torch reproduces conv2d)"""
    import torch
    import torch.nn.functional as F
    from pcp_amd import pack
    g = torch.Generator().manual_seed(5)
    w = torch.randn((100, 64, 3, 3), generator=g) * 0.05
    b = torch.randn((100,), generator=g)
    pws, bws, cpad = pack.pack_conv3x3_winograd_ws(w, b)
    assert tuple(pws.shape) == (64 // 2 + 2, cpad // 32, 2, 2, 2, 32, 4) and cpad == 128
    assert float(pws[-2:].abs().max()) == 0.0                                     # the prefetch overrun pad
    u = pack.unpack_winograd_ws(pws, 100)                                         # [cout, cin, 4, 4]
    pold, _, cpo = pack.pack_conv3x3_winograd(w, b)
    u_old = pold.permute(2, 0, 3, 1).reshape(cpo, 64, 4, 4)[:100]
    assert torch.equal(u, u_old)
    x = torch.randn((1, 64, 8, 8), generator=g)
    got = pack_eval.winograd_reference(x, pold, bws, 100)
    assert float((got - F.conv2d(x, w, b, padding=1)).abs().max()) < 1e-4


def test_winograd4h_weight_order_is_the_documented_permutation_and_dispatch_rule(monkeypatch):
    """include/pcp_hip.h: k_wino4h's weights are [cin/8][36][cout_pad/64][64 lanes][8] with lane l = 16 kq + c holding, at index 2 nb + ks,
    U[position][input channel 8 s + 4 ks + kq][output channel 64 n + 16 nb + c]; auto dispatch sends a layer to it up to 128 input channels
    once its 16 x 16-pixel items cover the chip"""
    import torch.nn as nn
    from pcdet.models import convnet
    from pcp_amd import pack
    torch.manual_seed(3)
    w, b = torch.randn(72, 16, 3, 3), torch.randn(72)
    pf, _bf, cp = pack.pack_conv3x3_winograd4f(w, b)                          # [2, 36, 128, 8]: U[s][pos][cout][k]
    ph, bh, cph = pack.pack_conv3x3_winograd4h(w, b)
    assert cph == cp == 128 and tuple(ph.shape) == (2, 36, 2, 64, 8) and torch.equal(bh, _bf)
    for (s, pos, n, lane, j) in [(0, 0, 0, 0, 0), (1, 35, 1, 63, 7), (0, 17, 1, 37, 5), (1, 4, 0, 22, 2)]:
        kq, c, nb, ks = lane >> 4, lane & 15, j >> 1, j & 1
        assert ph[s, pos, n, lane, j] == pf[s, pos, 64 * n + 16 * nb + c, 4 * ks + kq]
    # k_wino4c (include/pcp_hip.h): [cin/8][cout_pad/16][18 position pairs][64 lanes][4], lane l = 16 kq + c, index 2 e + ks =
    # U[position 2 q + e][input channel 8 s + 4 ks + kq][output channel 16 g + c]
    pc4, bc4, cpc4 = pack.pack_conv3x3_winograd4c(w, b)
    assert cpc4 == 128 and tuple(pc4.shape) == (2, 8, 18, 64, 4) and torch.equal(bc4, _bf)
    for (s, g, q, lane, j) in [(0, 0, 0, 0, 0), (1, 7, 17, 63, 3), (0, 4, 9, 37, 1), (1, 2, 3, 22, 2)]:
        kq, c, e, ks = lane >> 4, lane & 15, j >> 1, j & 1
        assert pc4[s, g, q, lane, j] == pf[s, 2 * q + e, 16 * g + c, 4 * ks + kq]
    pc = convnet.pack_conv_module(nn.Conv2d(128, 128, 3, padding=1, bias=False), None, relu=True)
    assert _choice(pc, (20, 64, 64, 128)) == 'winograd4c'                                 # 640 half-size items: the layer F(2x2) used to keep
    assert _choice(pc, (4, 64, 64, 128)) == 'winograd'                                    # 128 items: does not cover the chip
    wide = convnet.pack_conv_module(nn.Conv2d(384, 128, 3, padding=1, bias=False), None, relu=True)
    assert _choice(wide, (4, 128, 128, 384)) == 'winograd4f'                              # cin > 128: the eight-wave kernel
    monkeypatch.setenv('PCP_CONV_ALGO', 'winograd4h')
    assert _choice(wide, (4, 128, 128, 384)) == 'winograd4h'
    monkeypatch.setenv('PCP_CONV_ALGO', 'winograd4f')
    assert _choice(pc, (20, 64, 64, 128)) == 'winograd4f'


def _choice(pc, shape, in_ch_off=0):
    """the kernel conv_dispatch.choose_conv3x3 names for the packed layer on a map of `shape` (the launch allocates its output)"""
    from pcdet.models import convnet
    from pcp_amd import conv_dispatch
    B, H, W, ld = shape
    forms = convnet.Forms(*[f and f[2] for f in (pc.wino, pc.b3, pc.w4, pc.w4f, pc.mp)])
    return conv_dispatch.choose_conv3x3(conv_dispatch.conv_algo(), pc.cin, pc.cout, pc.stride, forms, B, H, W, ld, in_ch_off)


def _fused_f4(pc, shape, in_ch_off=0):
    return _choice(pc, shape, in_ch_off) in ('winograd4f', 'winograd4h', 'winograd4c')


def test_auto_dispatch_respects_the_fused_f4_kernels_own_limits(monkeypatch):
    """the fused F(4x4) kernel (csrc/wino4f.hip f4_geom) takes 16-byte aligned channel windows and at most 2 GiB of input
    (32-bit buffer-descriptor offsets); auto dispatch must fall through to the other kernels outside those limits instead of raising"""
    import torch.nn as nn
    from pcdet.models import convnet
    from pcp_amd import conv_dispatch
    conv = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    pc = convnet.pack_conv_module(conv, nn.BatchNorm2d(64).eval(), relu=True)
    assert pc.w4f is not None
    x = (4, 256, 256, 64)
    assert _fused_f4(pc, x)
    assert not _fused_f4(pc, x, 2)                                      # input window not 16-byte aligned
    assert not _fused_f4(pc, (4, 256, 256, 66))
    monkeypatch.setattr(conv_dispatch, 'WINOGRAD4F_MAX_INPUT_BYTES', 4 * 256 * 256 * 64 * 4 - 1)
    assert not _fused_f4(pc, x)                                         # over the byte limit: F(2x2) / direct take the layer
    monkeypatch.undo()
    big = (130, 256, 256, 64)                                           # the stacked car-maker pass at B = 26 frames: > 2 GiB
    assert 130 * 256 * 256 * 64 * 4 > 0x7fffffff and not _fused_f4(pc, big)
    # layers auto dispatch never sends to the fused kernel do not get its (4x sized) weight form packed
    wide = convnet.pack_conv_module(nn.Conv2d(768, 768, 3, padding=1, bias=False), None, relu=False)
    assert wide.w4 is not None and wide.w4f is None


def test_conv_dispatch_table_is_the_recorded_one():
    """tests/golden/conv_dispatch_table.json was recorded at the commit before pcp_amd/conv_dispatch.py existed (the file names it), by
    tests/golden/make_conv_dispatch_table.py through PackedConv.run and train_layers.fused_f4_choice with the ops functions stubbed out.  The
    same recorder on this code must give the same kernel, packed form, cout_pad and channel offset on every row, and the same fused-F(4x4)
    choice of the training step.  On the CPU the bf16-loop form is never packed (packing it needs a CUDA weight), so no row reaches the 'mp'
    branch; the bf16 training tests (tests/test_gpu_mp.py, test_gpu_train_ops.py) cover it on the GPU."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('make_conv_dispatch_table', os.path.join(GOLDEN, 'make_conv_dispatch_table.py'))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.TABLE) as f:
        doc = json.load(f)
    assert doc['launches'] == [r[0] for r in rec.launches(64, 64, 1)] and doc['fused_f4_launches'] == ['B%d %dx%d' % l for l in rec.f4_launches()]
    want, got = rec.decode(doc['dispatch']), rec.record_dispatch()
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (key, [(doc['launches'][i], w, g) for i, (w, g) in enumerate(zip(want[key], got[key])) if w != g])
    assert {c.split('/')[0] for c in doc['dispatch']['codes']} == {'conv3x3', 'conv3x3_winograd', 'conv3x3_winograd4', 'conv3x3_winograd4f',
                                                                 'conv3x3_winograd4h', 'conv3x3_winograd4c', 'conv3x3_bf16x3', 'pointwise'}
    want4, got4 = doc['fused_f4_choice'], rec.record_fused_f4()
    assert sorted(got4) == sorted(want4)
    for key in sorted(want4):
        assert got4[key] == want4[key], key


def test_train_conv_table_is_the_recorded_one():
    """tests/golden/train_conv_table.json was recorded at the commit before train_layers.TrainForms and conv_dispatch.choose_train_conv3x3
    existed (the file names it), by tests/golden/make_train_conv_table.py: ConvBNAct and _HeadBranches driven through their public surface
    over several optimizer steps with every ops / train_ops launch stubbed out and the group repack's library symbols faked.  The same
    recorder on this code must give the same launches in the same order with the same arguments, packed forms and group jobs on every row."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('make_train_conv_table', os.path.join(GOLDEN, 'make_train_conv_table.py'))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.TABLE) as f:
        doc = json.load(f)
    want, got = rec.decode(doc['table']), rec.record()
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (key, [(i, w, g) for i, (w, g) in enumerate(zip(want[key], got[key])) if w != g][:3],
                                       len(want[key]), len(got[key]))
    # a table that pins nothing would pass the above: the five kernel choices, the bf16 loop, both group launches and the stride-2 data
    # gradient are all in it
    assert rec.function_names(want) >= {'conv3x3', 'conv3x3_winograd', 'conv3x3_winograd4f', 'conv3x3_winograd4h', 'conv3x3_bf16x3',
                                        'mp_conv3x3', 'mp_pointwise', 'pack_conv3x3_group', 'mp_pack_conv3x3_group', 'dilate2x'}


def test_workspace_sizes_are_the_recorded_ones():
    """tests/golden/workspace_bytes.json was recorded by tests/golden/make_workspace_bytes.py with the library of the commit before
    PcpCarver (csrc/pcp_common.h) replaced the written-out carving lambdas (the file names it).  The same recorder on the built library
    must give the same value for every size query and argument set: the order and sizes of all workspace fields are unchanged."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('make_workspace_bytes', os.path.join(GOLDEN, 'make_workspace_bytes.py'))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.TABLE) as f:
        want = json.load(f)['table']
    got = rec.record()
    assert sorted(got) == sorted(want) and len(want) == 8
    for name in sorted(want):
        assert len(want[name]) >= 36, name
        assert got[name] == want[name], (name, [(w, g) for w, g in zip(want[name], got[name]) if w != g][:3])
        assert any(row[-1] > 256 for row in want[name]), name          # a table of refusals (0) or minimal sizes would pin nothing


def test_auto_resume_validates_a_checkpoint_before_anything_is_loaded(tmp_path):
    """tools/train.py: the newest checkpoint that is readable AND holds every model tensor at its shape is chosen; a torn file and a
    checkpoint of another architecture are skipped without touching the model (ADVICE r2 / VERDICT r3 item 9)."""
    import logging
    import sys
    import time
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'practical-collab-perception_amd', 'tools')
    sys.path.insert(0, tools)
    try:
        import train as train_tool
    finally:
        sys.path.remove(tools)
    model = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3), torch.nn.BatchNorm2d(8))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    log = logging.getLogger('resume-test')
    assert train_tool.choose_resume_checkpoint(model, tmp_path, log) is None
    good = tmp_path / 'checkpoint_epoch_1.pth'
    torch.save({'model_state': {k: v + 1 for k, v in before.items()}, 'epoch': 1, 'it': 10}, good)
    torch.save({'optimizer_state': {}}, tmp_path / 'checkpoint_epoch_1_optim.pth')          # side file: never a candidate
    time.sleep(0.02)
    other = tmp_path / 'checkpoint_epoch_2.pth'
    wrong = {k: v.clone() for k, v in before.items()}
    wrong['0.weight'] = torch.zeros(8, 4, 1, 1)
    torch.save({'model_state': wrong, 'epoch': 2, 'it': 20}, other)
    time.sleep(0.02)
    torn = tmp_path / 'checkpoint_epoch_3.pth'
    torn.write_bytes(good.read_bytes()[:200])
    now = time.time()
    for i, f in enumerate((good, other, torn)):
        os.utime(f, (now + i, now + i))
    assert train_tool.choose_resume_checkpoint(model, tmp_path, log) == str(good)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k])
    # with an optimizer to restore, its payload is validated too (the loader used to raise AFTER the model was overwritten):
    # the junk side file of `good` disqualifies it, a checkpoint with an extra tensor is refused (strict loading), one whose moments have
    # the flat buffer's size is taken, one of another size is not
    class _Opt:
        flat_p = torch.zeros(100)
    assert train_tool.choose_resume_checkpoint(model, tmp_path, log, _Opt()) is None
    sd = {k: v + 2 for k, v in before.items()}
    moments = lambda n: {'t': 3, 'exp_avg': torch.zeros(n), 'exp_avg_sq': torch.zeros(n), 'lr': 1e-3, 'mom': 0.9}
    fits, small, extra = tmp_path / 'checkpoint_epoch_4.pth', tmp_path / 'checkpoint_epoch_5.pth', tmp_path / 'checkpoint_epoch_6.pth'
    torch.save({'model_state': sd, 'epoch': 4, 'it': 40, 'optimizer_state': moments(100)}, fits)
    torch.save({'model_state': sd, 'epoch': 5, 'it': 50, 'optimizer_state': moments(64)}, small)
    torch.save({'model_state': dict(sd, stray=torch.zeros(1)), 'epoch': 6, 'it': 60, 'optimizer_state': moments(100)}, extra)
    for i, f in enumerate((fits, small, extra)):
        os.utime(f, (now + 10 + i, now + 10 + i))
    assert train_tool.choose_resume_checkpoint(model, tmp_path, log, _Opt()) == str(fits)
    assert train_tool.choose_resume_checkpoint(model, tmp_path, log) == str(small)         # no optimizer to restore: only the model half counts


def test_vectorised_warp_thetas_equal_the_reference_arithmetic_bit_for_bit():
    """pcp_amd/fusion_host.py::warp_thetas (all (agent, frame) pairs of a forward in one numpy pass) against warp_theta, the torch-CPU
    restatement of the reference's transform_bev_img parameter arithmetic (v2x_fusion_disco.py:32-35): 3 000 random rigid poses, two map
    geometries, every one of the six floats identical -- including the fused (2, 2) @ (2, 1) product, which a plain mul + add gets wrong
    in a quarter of the cases"""
    from pcp_amd import fusion_host as fh
    rng = np.random.RandomState(11)
    poses = []
    for _ in range(3000):
        a = rng.uniform(-np.pi, np.pi)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = rng.uniform(-90, 90, 3)
        poses.append(T)
    for h, pc_min, pix in ((128, -51.2, 0.8), (16, -12.8, 1.6)):
        assert fh._calibrated(h, pc_min, pix)                       # one of the known rounding forms reproduces this machine's small torch matmul
        fast = fh.warp_thetas(poses, h, h, pc_min, pix)
        slow = [fh.warp_theta(fh.ego_se3_agent(T), h, h, pc_min, pix) for T in poses]
        assert fast == slow
    # the rounding of that product depends on the host's BLAS (fused chain on this container, mul + add on the MI355X boxes' EPYC): the form
    # the calibration picked reproduces torch, and the other candidate forms do NOT (so the choice is doing something)
    form = fh._form(128, -51.2, 0.8)
    ref = np.array(fh.warp_thetas(poses, 128, 128, -51.2, 0.8), dtype=np.float32)
    assert np.array_equal(fh._thetas_numpy(poses, 128, -51.2, 0.8, form), ref)
    for other in fh._FORMS:
        if other != form:
            assert (fh._thetas_numpy(poses, 128, -51.2, 0.8, other) != ref).any(axis=1).mean() > 0.05, other


def test_deferred_batchnorm_counters_are_flushed_before_state_dict_and_dropped_on_load():
    """num_batches_tracked increments of the training path are collected and applied once per optimizer step; a state_dict()
    taken between a forward and the step must still see them, and a load_state_dict() must not have older increments added on top."""
    import torch.nn as nn
    from pcdet.models.packed import PackedModule
    from pcp_amd import train_layers as tl

    class M(PackedModule):
        def __init__(self):
            super().__init__()
            self.bn = nn.BatchNorm2d(4)
    m = M()
    tl.bump_batches_tracked(m.bn)
    tl.bump_batches_tracked(m.bn)
    sd = m.state_dict()
    assert int(sd['bn.num_batches_tracked']) == 2
    tl.bump_batches_tracked(m.bn)                                # a warm-up forward, then a checkpoint is loaded
    sd = {k: v.clone() for k, v in sd.items()}
    sd['bn.num_batches_tracked'] = torch.tensor(7)
    m.load_state_dict(sd)
    tl.StepClock.tick()
    assert int(m.bn.num_batches_tracked) == 7


REF_CALLERS = ['tools/test.py', 'tools/train.py', 'tools/eval_utils/eval_utils.py', 'tools/train_utils/train_utils.py']


@pytest.mark.skipif(not os.path.isdir('/root/reference'), reason='build container only: reads the reference callers (never on the GPU box)')
def test_the_references_unchanged_callers_bind_to_this_package():
    """INTEGRATION.md section A invites a maintainer to keep the reference's own tools/ scripts and swap the package underneath.  By AST, for
    the four caller files: (1) every name they import from pcdet.* / eval_utils / train_utils.* exists in this build's module of the same
    path; (2) every attribute they read off an imported module (common_utils.create_logger, cfg.ROOT_DIR is data, ...) exists for the
    imported utility modules; (3) every call of a boundary function (train_model, build_network, build_dataloader, build_optimizer,
    build_scheduler, eval_one_epoch, model_fn_decorator, load_data_to_gpu) passes only keywords -- and no more positionals -- than this
    build's function of that name accepts."""
    import ast
    import importlib
    import inspect
    import sys
    tools = os.path.join(REPO, 'practical-collab-perception_amd', 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    boundary = {}
    checked_calls = 0
    for rel in REF_CALLERS:
        tree = ast.parse(open(os.path.join('/root/reference', rel)).read())
        imported_mods = {}
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split('.')[0] in ('pcdet', 'eval_utils', 'train_utils'):
                mod = importlib.import_module(node.module)
                for alias in node.names:
                    if not hasattr(mod, alias.name):
                        try:                                                    # `from eval_utils import eval_utils`: a submodule
                            importlib.import_module(node.module + '.' + alias.name)
                        except ImportError:
                            pass
                    assert hasattr(mod, alias.name), '%s: `from %s import %s` does not resolve in this build' % (rel, node.module, alias.name)
                    obj = getattr(mod, alias.name)
                    if inspect.ismodule(obj):
                        imported_mods[alias.asname or alias.name] = obj
                    elif callable(obj):
                        boundary[alias.asname or alias.name] = obj
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in imported_mods:
                mod = imported_mods[node.value.id]
                if node.attr == 'commu_utils' or mod.__name__.endswith('commu_utils'):
                    continue
                assert hasattr(mod, node.attr), '%s: %s.%s is used by the reference caller and missing here' % (rel, mod.__name__, node.attr)
                if callable(getattr(mod, node.attr)):
                    boundary['%s.%s' % (node.value.id, node.attr)] = getattr(mod, node.attr)
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            name = node.func.id if isinstance(node.func, ast.Name) else (
                '%s.%s' % (node.func.value.id, node.func.attr) if isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) else None)
            fn = boundary.get(name)
            if fn is None or inspect.isclass(fn):
                continue
            try:
                sig = inspect.signature(fn)
            except (TypeError, ValueError):
                continue
            params = sig.parameters
            if any(p.kind == p.VAR_KEYWORD for p in params.values()):
                accepted = None
            else:
                accepted = {n for n, p in params.items() if p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)}
            for kw in node.keywords:
                if kw.arg is not None and accepted is not None:
                    assert kw.arg in accepted, '%s:%d %s(... %s=...) is not accepted by this build (%s)' % (rel, node.lineno, name, kw.arg, sig)
            n_pos = sum(1 for p in params.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD))
            if not any(p.kind == p.VAR_POSITIONAL for p in params.values()):
                assert len(node.args) <= n_pos, '%s:%d %s takes %d positionals here, the reference passes %d' % (rel, node.lineno, name, n_pos, len(node.args))
            checked_calls += 1
    assert {'train_model', 'build_network', 'build_dataloader', 'build_optimizer', 'build_scheduler', 'model_fn_decorator',
            'load_data_to_gpu'} <= set(boundary), sorted(boundary)
    assert 'eval_utils.eval_one_epoch' in boundary and checked_calls >= 12, (checked_calls, sorted(boundary))


def test_option_table_round_trip_and_env_mapping(monkeypatch):
    """pcp_set_option / pcp_get_option need no GPU: defaults read -1 ("built-in rule"), a set value reads back, a negative value restores the
    rule, an unknown option is refused -- and the library itself never reads the environment (the Python host maps PCP_* once at load)."""
    import ctypes
    from pcp_amd import lib
    L = lib.load()
    assert set(lib.OPTIONS.values()) == set(range(len(lib.OPTIONS)))
    for name, idx in lib.OPTIONS.items():
        assert L.pcp_get_option(idx) == -1, name
    prev = lib.set_option('pfn_crowd', 64)
    assert prev is None and L.pcp_get_option(lib.OPTIONS['pfn_crowd']) == 64
    assert lib.set_option('pfn_crowd', None) == 64 and L.pcp_get_option(lib.OPTIONS['pfn_crowd']) == -1
    assert L.pcp_set_option(len(lib.OPTIONS), 1) != 0 and L.pcp_set_option(-1, 1) != 0 and L.pcp_get_option(99) == -1
    monkeypatch.setenv('PCP_PFN_CROWD', '128')                    # set AFTER the load: the library must not see it
    assert L.pcp_get_option(lib.OPTIONS['pfn_crowd']) == -1
    # no source of the library calls getenv (the one import of the symbol in the shared object comes from a rocPRIM header -- hipcub's
    # DeviceRadixSort inside the training entry pcp_hunter_losses reads ROCPRIM_USE_ATOMIC_BLOCK_ID, rocprim/device/detail/ordered_block_id.hpp)
    csrc = os.path.join(REPO, 'practical-collab-perception_amd', 'csrc')
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.h')):
            assert 'getenv' not in open(os.path.join(csrc, f)).read(), f
    # the export entry point validates its arguments without touching a device
    g = lib.Grid(-51.2, -51.2, -8.0, 0.2, 0.2, 8.0, 512, 512, 1)
    assert L.pcp_pillar_index_export(ctypes.byref(g), None, 10, 5, None, None, None, None, None, None) != 0
    assert L.pcp_pillar_index_export(ctypes.byref(g), ctypes.c_void_p(256), 10, 2, None, None, None, None, None, None) != 0       # num_raw < 3


def test_rank_affinity_slices_whole_cores(monkeypatch):
    from pcp_amd import hostcpu
    assert hostcpu.cpu_list([0, 1, 2, 3, 8, 10, 11]) == '0-3,8,10-11' and hostcpu.cpu_list([]) == ''
    avail = sorted(os.sched_getaffinity(0))
    try:
        cores = hostcpu._physical_cores(avail)
        assert sorted(c for core in cores for c in core) == avail and all(core == sorted(core) for core in cores)
        assert hostcpu.pin_rank_to_cpus(0, 1) == avail                                  # one rank: mask untouched
        assert hostcpu.pin_rank_to_cpus(5, 2) == avail                                  # nonsense rank: mask untouched
        monkeypatch.setenv('PCP_AFFINITY', '0')
        assert hostcpu.pin_rank_to_cpus(0, 2) == avail
        monkeypatch.delenv('PCP_AFFINITY')
        if len(cores) >= 2:
            mine = hostcpu.pin_rank_to_cpus(1, 2)
            per = len(cores) // 2
            assert mine == sorted(c for core in cores[per:2 * per] for c in core) and sorted(os.sched_getaffinity(0)) == mine
    finally:
        os.sched_setaffinity(0, avail)
