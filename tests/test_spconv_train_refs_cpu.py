"""The float64 autograd restatement of tests/spconv_train_refs.py pinned on the CPU: a hand-computed two-site case, torch.autograd.gradcheck
on a 3 x 3 x 3 grid, the brute-force inverse table, the batch-statistics BatchNorm against torch's own, and the conditioning of the seeded
whole-backbone case.  No GPU."""
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (os.path.join(REPO, 'tests'), os.path.join(REPO, 'practical-collab-perception_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import spconv_refs as sr  # noqa: E402
import spconv_train_refs as tr  # noqa: E402


def test_two_sites_by_hand():
    """sites a = (0, 1, 1, 1) and b = (0, 1, 1, 2) on a 3 x 3 x 3 grid, submanifold 3 x 3 x 3: b is a's neighbour at offset (1, 1, 2) = k 14,
    a is b's at (1, 1, 0) = k 12, each is its own at k 13.  With x = [[1, 2], [3, 5]], dy = [[7], [11]]:
      dW[13] = 7 x_a + 11 x_b = [40, 69]; dW[14] = 7 x_b = [21, 35]; dW[12] = 11 x_a = [11, 22]
      dx_a = 7 W[13] + 11 W[12], dx_b = 7 W[14] + 11 W[13]"""
    coords = np.array([[0, 1, 1, 1], [0, 1, 1, 2]], np.int32)
    x = np.array([[1., 2.], [3., 5.]])
    dy = np.array([[7.], [11.]])
    w = np.arange(27 * 2, dtype=np.float64).reshape(1, 3, 3, 3, 2) + 1.0
    g = tr.conv_grads_ref(x, coords, (1, 3, 3, 3), w, dy)
    dw = g['dw'].reshape(27, 2)
    want = np.zeros((27, 2))
    want[13], want[14], want[12] = [40, 69], [21, 35], [11, 22]
    assert np.array_equal(dw, want)
    wk = w.reshape(27, 2)
    assert np.array_equal(g['dx'], np.stack([7 * wk[13] + 11 * wk[12], 7 * wk[14] + 11 * wk[13]]))
    assert np.array_equal(g['dw_abs'], np.abs(g['dw'])) and np.array_equal(g['dx_abs'], g['dx'])      # all factors positive here
    nbr = sr.subm_nbr_brute(coords)
    assert nbr[14, 0] == 1 and nbr[12, 1] == 0 and list(nbr[13]) == [0, 1] and (nbr >= 0).sum() == 4
    inv = tr.inverse_table_brute(nbr, 2)
    assert np.array_equal(inv, nbr[::-1])                                                               # the mirrored-offset identity


def test_gradcheck_on_a_3x3x3_grid():
    rs = np.random.RandomState(0)
    lin = np.flatnonzero(rs.rand(27) < 0.5)
    coords = np.stack([np.zeros_like(lin), lin // 9, (lin // 3) % 3, lin % 3], 1).astype(np.int32)
    x = torch.from_numpy(rs.randn(len(coords), 2)).requires_grad_(True)
    w = torch.from_numpy(rs.randn(3, 3, 3, 3, 2)).requires_grad_(True)
    b = torch.from_numpy(rs.randn(3)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, w, b: tr.sparse_conv_t(x, coords, (1, 3, 3, 3), w, b), (x, w, b))
    oc = sr.strided_out_coords(coords, (1, 3, 3, 3), 3, 2, 1)
    assert torch.autograd.gradcheck(lambda x, w: tr.sparse_conv_t(x, coords, (1, 3, 3, 3), w, None, 3, 2, 1, oc), (x, w))
    # the forward is sparse_conv_ref's
    y, _ = sr.sparse_conv_ref(x.detach().numpy(), coords, (1, 3, 3, 3), w.detach().numpy(), b.detach().numpy())
    assert np.allclose(tr.sparse_conv_t(x, coords, (1, 3, 3, 3), w, b).detach().numpy(), y, rtol=0, atol=1e-12)


def test_inverse_table_of_a_strided_geometry():
    rs = np.random.RandomState(1)
    lin = np.flatnonzero(rs.rand(5 * 6 * 7) < 0.3)
    coords = np.stack([np.zeros_like(lin), lin // 42, (lin // 7) % 6, lin % 7], 1).astype(np.int32)
    oc = sr.strided_out_coords(coords, (1, 5, 6, 7), 3, 2, 1)
    nbr = sr.nbr_brute(coords, oc, 3, 2, 1)
    inv = tr.inverse_table_brute(nbr, len(coords))
    assert (inv >= 0).sum() == (nbr >= 0).sum()
    for k, i in zip(*np.nonzero(inv >= 0)):
        assert nbr[k, inv[k, i]] == i


def test_batch_statistics_batchnorm_is_torchs():
    rs = np.random.RandomState(2)
    y = torch.from_numpy(rs.randn(37, 5))
    bn = torch.nn.BatchNorm1d(5, eps=tr.BN_EPS, momentum=tr.BN_MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rs.rand(5) + 0.5))
        bn.bias.copy_(torch.from_numpy(rs.randn(5)))
        bn.running_var.copy_(torch.from_numpy(rs.rand(5) + 0.5))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    out, rm2, rv2 = tr.bn_train_t(y, bn.weight.detach(), bn.bias.detach(), rm, rv)
    want = bn(y)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    assert torch.allclose(rm2, bn.running_mean, rtol=0, atol=1e-14) and torch.allclose(rv2, bn.running_var, rtol=0, atol=1e-14)


def _state_shapes():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d import VoxelResBackBone8x
    D, H, W = tr.TRAIN_GRID
    bb = VoxelResBackBone8x(EasyDict({'NAME': 'VoxelResBackBone8x', 'HIP_TRAIN': True}), input_channels=11, grid_size=np.asarray([W, H, D]))
    return {k: tuple(v.shape) for k, v in bb.state_dict().items()}


def test_seeded_backbone_case_is_conditioned():
    """no pre-ReLU value of the batch-statistics restatement within TRAIN_MARGIN of zero; every ReLU has rows on both sides; conv_out has rows;
    every parameter has a gradient and the blocks' conv biases have a zero one"""
    st, feats, coords, dcanvas, want, pre = tr.second_train_case(_state_shapes())
    assert len(pre) == 21 and want['rows'] >= 8
    near = min(float(np.abs(p).min()) for p in pre)
    assert near >= tr.TRAIN_MARGIN, near
    assert all(0.05 < float((p > 0).mean()) < 0.95 for p in pre)
    assert want['spatial_features'].shape == (2, 128, 4, 4) and np.abs(want['spatial_features']).max() > 0.1
    g = want['grads']
    assert set(g) == {k for k in st if not k.endswith('num_batches_tracked') and 'running' not in k}
    for k, v in g.items():
        assert np.isfinite(v).all()
        if k.endswith('conv1.bias') or k.endswith('conv2.bias'):
            assert np.abs(v).max() <= 1e-9 * max(np.abs(g[k[:-4] + 'weight']).max(), 1.0), k
        else:
            assert np.abs(v).max() > 0, k
