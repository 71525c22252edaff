"""SC backbone training, CPU side: the fixtures g22_sc_block_train and g22_sc_backbone_train (tests/golden/make_golden_nusc_sc_train.py)
load and describe the bottleneck and the backbone this package builds, and the inverse nearest-index ranges the gate backward gathers over partition the map."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import nusc_sc_refs as refs
from helpers import GOLDEN, load_golden

MiB = 1 << 20


def test_block_fixture_loads_and_describes_the_bottleneck():
    from pcdet.models.backbones_2d.sc_conv_backbone import SCBottleneck
    assert os.path.getsize(os.path.join(GOLDEN, 'g22_sc_block_train.npz')) < MiB
    g = load_golden('g22_sc_block_train.npz')
    cases = g['meta']['cases']
    assert set(cases) == {'p32', 'p64'}
    assert cases['p32']['shape'] == [2, 32, 30, 14] and cases['p64']['shape'] == [2, 64, 8, 12]
    for tag, c in cases.items():
        blk = SCBottleneck(c['planes'], c['planes'], partial(torch.nn.BatchNorm2d, eps=c['bn_eps'], momentum=c['bn_momentum']))
        mine = {k: list(v.shape) for k, v in blk.state_dict().items()}
        assert mine == c['state_shapes'], tag
        assert c['relu_probe_deviation'] <= 1e-2 and c['min_relu_gap'] >= 1e-4
        assert list(g[tag + '/out'].shape) == c['shape'] and list(g[tag + '/dx'].shape) == c['shape']
        params = dict(blk.named_parameters())
        assert set(c['param_names']) == set(params)
        for n, p in params.items():
            assert g['%s/g/%s' % (tag, n)].shape == tuple(p.shape), (tag, n)
        for k in mine:
            if 'running_' in k:
                assert g['%s/bn/%s' % (tag, k)].shape == tuple(mine[k]), (tag, k)


def test_backbone_fixture_loads_and_describes_the_stride4_backbone():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.sc_conv_backbone import SCConvBackbone2dStride4
    assert os.path.getsize(os.path.join(GOLDEN, 'g22_sc_backbone_train.npz')) < MiB
    g = load_golden('g22_sc_backbone_train.npz')
    meta = g['meta']
    bb = SCConvBackbone2dStride4(EasyDict(meta['cfg']), meta['input_channels'])
    mine = {k: list(v.shape) for k, v in bb.state_dict().items()}
    assert mine == meta['state_shapes']
    assert meta['relu_probe_deviation'] <= 1e-2
    B, _c, H, W = meta['canvas']
    assert (H // 2) % 4 and (H // 4) % 4 and (W // 2) % 4 and (W // 4) % 4        # stem and main-pass sides are no multiples of 4
    assert g['out'].shape == (B, meta['cfg']['NUM_BEV_FEATURES'], H // 4, W // 4) and list(g['dx'].shape) == meta['canvas']
    params = dict(bb.named_parameters())
    assert meta['param_names'] == list(params) and g['grad_digest'].shape == (len(params), 3)
    for n, p in params.items():
        assert g['g/' + n].size == (p.numel() if p.numel() <= meta['whole_cap'] else 1024), n
    for k in mine:
        if 'running_' in k:
            assert g['bn/' + k].shape == tuple(mine[k]), k
    assert bb.conv_out[1].eps == 1e-5 and bb.conv_out[1].momentum == 0.1 and bb.stem[0][1].eps == 1e-3


def _pairs():
    for h in range(4, 131):
        yield h, h // 4
    for sh in (1, 3, 7, 16, 65):
        yield sh, sh
        yield 2 * sh, sh


def test_inverse_nearest_ranges_partition_the_axis():
    """the float64 statement, the forward's float32 index and the kernel's guess-and-walk agree for every (h, h // 4) with 4 <= h <= 130 and
    for the equal-size and exact-2x cases: the ranges tile range(h) without gap or overlap and each is exactly the preimage of its source"""
    for h, sh in _pairs():
        r = refs.inverse_ranges(h, sh)
        assert r[0, 0] == 0 and r[-1, 1] == h and np.array_equal(r[1:, 0], r[:-1, 1]) and (r[:, 1] > r[:, 0]).all(), (h, sh)
        src = refs.nearest_src(h, sh)
        for k in range(sh):
            assert np.array_equal(np.nonzero(src == k)[0], np.arange(r[k, 0], r[k, 1])), (h, sh, k)
        assert np.array_equal(refs.kernel_ranges(h, sh), r), (h, sh)


def test_nearest_src_is_torch_interpolate():
    """ties the numpy index the partition test is stated against to what F.interpolate does"""
    for h, sh in list(_pairs())[::7] + [(30, 7), (15, 3), (14, 3), (7, 1), (5, 1)]:
        want = torch.nn.functional.interpolate(torch.arange(sh, dtype=torch.float32).view(1, 1, sh, 1), size=(h, 1)).view(-1).long().numpy()
        assert np.array_equal(refs.nearest_src(h, sh), want), (h, sh)
