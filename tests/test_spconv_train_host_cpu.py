"""Host side of the sparse-conv training path, no GPU: the workspace sizes of pcp_spconv3d_wgrad against tests/golden/spconv_train_workspace_bytes.json,
the data-gradient weight packing, the HIP_TRAIN switch and the declarations of the new entry points."""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (os.path.join(REPO, 'tests'), os.path.join(REPO, 'practical-collab-perception_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from pcp_amd import lib, ops  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'spconv_train_workspace_bytes.json')
NEW_SYMBOLS = ['pcp_spconv_invert_nbr', 'pcp_spconv3d_wgrad_workspace_bytes', 'pcp_spconv3d_wgrad', 'pcp_spconv_dense_backward']


def workspace_cases():
    """(n_out, num_offsets, cin, cout, chunk_rows)"""
    pairs = [(5, 16), (11, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
    return [(n, k, ci, co, ch) for (ci, co) in pairs for (n, k) in ((0, 27), (1, 27), (1023, 27), (1025, 3), (32768, 27), (32769, 27), (653634, 27))
            for ch in (0, 16, 4096)]


def test_workspace_bytes_match_the_recorded_table():
    L = lib.load()
    table = json.load(open(GOLDEN))
    cases = workspace_cases()
    assert len(table) == len(cases)
    for case, rec in zip(cases, table):
        assert list(case) == rec[:5] and L.pcp_spconv3d_wgrad_workspace_bytes(*case) == rec[5], (case, rec)


def test_workspace_rule():
    """the rule: at most 32 chunks of at least 1024 rows, so never more than 27 x 32 x Cout x cin_pad floats (four times that where four waves split
    the rows of a 16-channel output)"""
    L = lib.load()
    assert L.pcp_spconv3d_wgrad_workspace_bytes(653634, 27, 128, 128, 0) == 27 * 32 * 128 * 128 * 4
    assert L.pcp_spconv3d_wgrad_workspace_bytes(10 ** 7, 27, 128, 128, 0) == 27 * 32 * 128 * 128 * 4
    assert L.pcp_spconv3d_wgrad_workspace_bytes(1024, 27, 128, 128, 0) == 27 * 128 * 128 * 4
    assert L.pcp_spconv3d_wgrad_workspace_bytes(1025, 27, 11, 16, 0) == 27 * 2 * 4 * 16 * 16 * 4
    assert L.pcp_spconv3d_wgrad_workspace_bytes(1025, 27, 16, 32, 0) == 27 * 2 * 2 * 32 * 16 * 4
    for bad in ((100, 27, 16, 64, 0), (100, 27, 32, 16, 0), (100, 28, 16, 16, 0), (100, 27, 16, 16, 24), (-1, 27, 16, 16, 0), (100, 27, 2, 16, 0)):
        assert L.pcp_spconv3d_wgrad_workspace_bytes(*bad) == 0, bad


def test_entry_points_are_declared():
    text = open(os.path.join(REPO, 'include', 'pcp_hip_train.h')).read()
    for name in NEW_SYMBOLS:
        assert name + '(' in text and name in lib.SYMBOLS and hasattr(lib.load(), name), name


def test_data_gradient_weight_packing():
    rs = np.random.RandomState(0)
    w = torch.from_numpy(rs.randn(4, 3, 3, 3, 5).astype(np.float32))
    plain, mirrored = ops.spconv_pack_weight_dgrad(w, mirror=False), ops.spconv_pack_weight_dgrad(w, mirror=True)
    assert tuple(plain.shape) == (27, 5, 4) and plain.is_contiguous() and mirrored.is_contiguous()
    wk = w.reshape(4, 27, 5)
    for k in (0, 5, 13, 26):
        assert torch.equal(plain[k], wk[:, k].t()) and torch.equal(mirrored[k], wk[:, 26 - k].t())
    w3 = torch.from_numpy(rs.randn(4, 3, 1, 1, 5).astype(np.float32))
    assert torch.equal(ops.spconv_pack_weight_dgrad(w3, mirror=False)[2], w3.reshape(4, 3, 5)[:, 2].t())
    assert (32, 16) in ops.SPCONV_CHANNEL_PAIRS and (64, 32) in ops.SPCONV_CHANNEL_PAIRS and (128, 64) in ops.SPCONV_CHANNEL_PAIRS


def test_the_switch_allows_train_and_its_absence_refuses():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d import VoxelResBackBone8x
    from pcdet.models.backbones_3d.vfe import DynamicMeanVFE
    grid = np.asarray([32, 32, 24])
    args = dict(num_point_features=11, voxel_size=[0.1, 0.1, 0.2], grid_size=grid, point_cloud_range=[0, 0, 0, 3.2, 3.2, 4.8])
    for cfg, ok in ((EasyDict({'NAME': 'x'}), False), (EasyDict({'NAME': 'x', 'HIP_TRAIN': False}), False), (EasyDict({'NAME': 'x', 'HIP_TRAIN': True}), True)):
        for m in (VoxelResBackBone8x(cfg, input_channels=11, grid_size=grid), DynamicMeanVFE(cfg, **args)):
            if ok:
                assert m.train().training and not m.eval().training
            else:
                with pytest.raises(NotImplementedError, match='inference only'):
                    m.train()
                assert not m.eval().training
    # the spconv modules themselves keep refusing a training-mode forward
    from pcp_amd import spconv
    with pytest.raises(NotImplementedError, match='inference only'):
        spconv.SubMConv3d(16, 16, 3).train()(None)
