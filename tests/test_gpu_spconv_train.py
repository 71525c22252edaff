"""The training kernels of the sparse 3D convolution (csrc/spconv3d_train.hip) on the GPU against the float64 autograd restatement of
tests/spconv_train_refs.py: the inverse neighbour table, the weight gradient, the data gradient (pcp_spconv3d on the mirrored / inverse
table), the gradient of dense().  Tiny grids: B = 3 with an empty middle frame, spatial (9, 12, 12), occupancy 0.1."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (os.path.join(REPO, 'tests'), os.path.join(REPO, 'practical-collab-perception_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import spconv_refs as sr  # noqa: E402
import spconv_train_refs as tr  # noqa: E402
from pcp_amd import lib, ops  # noqa: E402
from pcp_amd import train_ops as tops  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B, SPATIAL = 3, (9, 12, 12)
SHAPE4 = (B,) + SPATIAL
PAIRS = [(5, 16), (11, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]      # forward (Cin, Cout)
SUBM = (3, 1, 1)
STRIDED = [(3, 2, 1), (3, 2, (0, 1, 1)), ((3, 1, 1), (2, 1, 1), 0), ((3, 1, 1), (2, 1, 1), 1)]
GEOMS = [SUBM] + STRIDED
GEOM_IDS = ['subm', 's2p1', 's2p011', 'out_pad0', 'out_pad1']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sites():
    """distinct sites of frames 0 and 2 (frame 1 is empty) in the mean VFE's order (b, x, y, z): not the linear one"""
    rs = np.random.RandomState(5)
    D, H, W = SPATIAL
    rows = []
    for b in (0, 2):
        lin = np.flatnonzero(rs.rand(D * H * W) < 0.1)
        rows.append(np.stack([np.full(len(lin), b), lin // (H * W), (lin // W) % H, lin % W], 1))
    c = np.concatenate(rows, 0)
    return np.ascontiguousarray(c[np.lexsort((c[:, 1], c[:, 2], c[:, 3], c[:, 0]))].astype(np.int32))


SITES = _sites()
_GEOM_CACHE = {}


def geometry(geom, coords=None):
    """-> dict(coords, out_coords, nbr (brute force), subm) of one layer geometry over `coords` (default: the shared set); computed once"""
    key = (GEOMS.index(geom), None if coords is None else coords.tobytes())
    if key not in _GEOM_CACHE:
        c = SITES if coords is None else coords
        if geom == SUBM:
            g = dict(coords=c, out_coords=c, nbr=sr.subm_nbr_brute(c), subm=True)
        else:
            oc = sr.strided_out_coords(c, SHAPE4, *geom)
            g = dict(coords=c, out_coords=oc, nbr=sr.nbr_brute(c, oc, *geom), subm=False)
        g['geom'] = geom
        _GEOM_CACHE[key] = g
    return _GEOM_CACHE[key]


def gpu_tables(g):
    """the library's own tables for the geometry: (nbr, table of the data gradient)"""
    c = dev(g['coords'])
    table = ops.spconv_table(c, B, SPATIAL)
    if g['subm']:
        nbr = ops.spconv_build_subm(c, table)
        return nbr, nbr
    oc, nbr, _ = ops.spconv_build_strided(c, table, *g['geom'])
    assert np.array_equal(oc.cpu().numpy(), g['out_coords'])
    return nbr, tops.spconv_invert_nbr(nbr, len(g['coords']))


def gpu_grads(g, x, dy, w, chunk_rows=0, want_dx=True):
    """dW by pcp_spconv3d_wgrad into a NaN-filled buffer, dx by pcp_spconv3d with the data-gradient weights"""
    nbr, back = gpu_tables(g)
    cout, cin = w.shape[0], w.shape[-1]
    dw = torch.full(tuple(w.shape), float('nan'), dtype=torch.float32, device='cuda')
    tops.spconv3d_wgrad(dev(x), dev(dy), nbr, dw, chunk_rows=chunk_rows)
    dx = None
    if want_dx and cin >= 16:
        wd = ops.spconv_pack_weight_dgrad(dev(w), mirror=g['subm'])
        assert tuple(wd.shape) == (nbr.shape[0], cin, cout)
        dx = ops.spconv3d(dev(dy), back, wd, torch.zeros(cin, device='cuda'))
    torch.cuda.synchronize()
    return dw.cpu().numpy(), None if dx is None else dx.cpu().numpy()


def int_case(g, cin, cout, seed):
    rs = np.random.RandomState(seed)
    K = g['nbr'].shape[0]
    kshape = g['geom'][0] if isinstance(g['geom'][0], tuple) else (g['geom'][0],) * 3
    assert K == kshape[0] * kshape[1] * kshape[2]
    x = rs.randint(-2, 3, (len(g['coords']), cin)).astype(np.float32)
    dy = rs.randint(-2, 3, (len(g['out_coords']), cout)).astype(np.float32)
    w = rs.randint(-2, 3, (cout,) + kshape + (cin,)).astype(np.float32)
    return x, dy, w


def ref_grads(g, x, dy, w):
    k, s, p = g['geom']
    return tr.conv_grads_ref(x, g['coords'], SHAPE4, w, dy, k, s, p, None if g['subm'] else g['out_coords'])


@pytest.mark.parametrize('geom', STRIDED, ids=GEOM_IDS[1:])
def test_inverse_table_entry_for_entry(geom):
    g = geometry(geom)
    nbr, inv = gpu_tables(g)
    assert np.array_equal(nbr.cpu().numpy(), g['nbr'])
    want = tr.inverse_table_brute(g['nbr'], len(g['coords']))
    assert inv.dtype == torch.int32 and np.array_equal(inv.cpu().numpy(), want)
    assert (want >= 0).sum() == (g['nbr'] >= 0).sum() > 0


def test_submanifold_table_is_its_own_mirrored_inverse():
    g = geometry(SUBM)
    nbr, _ = gpu_tables(g)
    got = nbr.cpu().numpy()
    assert np.array_equal(got, sr.subm_nbr_brute(SITES))
    assert np.array_equal(tr.inverse_table_brute(got, len(SITES)), got[::-1])              # nbr[k][j] == i exactly when nbr[26 - k][i] == j
    assert np.array_equal(tops.spconv_invert_nbr(nbr, len(SITES)).cpu().numpy(), got[::-1])


@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize('cin,cout', PAIRS)
def test_small_integers_are_exact(cin, cout, geom):
    """sums of products of integers in [-2, 2]: below 27 * 128 * 4 < 2^24, so fp32 in any order is exact.  The data gradient of the forward pair
    (Cin, Cout) runs pcp_spconv3d's pair (Cout -> Cin): 32 -> 16, 64 -> 32 and 128 -> 64 among them."""
    g = geometry(geom)
    x, dy, w = int_case(g, cin, cout, 100 + cin + cout)
    want = ref_grads(g, x, dy, w)
    dw, dx = gpu_grads(g, x, dy, w)
    assert np.abs(want['dw']).max() > 0 and np.array_equal(dw.astype(np.float64), want['dw'])
    if cin >= 16:
        assert np.abs(want['dx']).max() > 0 and np.array_equal(dx.astype(np.float64), want['dx'])


@pytest.mark.parametrize('geom', [SUBM, STRIDED[2]], ids=['subm', 'out_pad0'])
def test_one_hot_pins_every_offset(geom):
    """one row of x and one row of dy set, a pair that meets at offset k only: dW is 1 at (co, k, ci) and 0 elsewhere, for each k"""
    g = geometry(geom)
    nbr_d, _ = gpu_tables(g)
    K = g['nbr'].shape[0]
    assert K == (27 if geom == SUBM else 3)
    for k in range(K):
        js = np.flatnonzero(g['nbr'][k] >= 0)
        assert len(js), k
        j = int(js[len(js) // 2])
        i = int(g['nbr'][k, j])
        ci, co = (3 * k + 1) % 16, (5 * k + 2) % 16
        x = np.zeros((len(g['coords']), 16), np.float32)
        dy = np.zeros((len(g['out_coords']), 16), np.float32)
        x[i, ci], dy[j, co] = 1.0, 1.0
        dw = torch.full((16, K, 16), float('nan'), device='cuda')
        tops.spconv3d_wgrad(dev(x), dev(dy), nbr_d, dw)
        want = np.zeros((16, K, 16), np.float32)
        want[co, k, ci] = 1.0
        assert np.array_equal(dw.cpu().numpy(), want), k


_WORST = {}


@pytest.mark.parametrize('geom', [SUBM, STRIDED[0]], ids=['subm', 's2p1'])
@pytest.mark.parametrize('cin,cout', PAIRS)
def test_random_floats_within_the_fp32_summation_bound(cin, cout, geom):
    """every element within (n_terms + 2) 2^-24 sum |terms|; dW: the rows contributing at that offset, dx: K * Cout terms"""
    g = geometry(geom)
    rs = np.random.RandomState(7 + cin + cout)
    K = g['nbr'].shape[0]
    x = rs.uniform(-1, 1, (len(g['coords']), cin)).astype(np.float32)
    dy = rs.uniform(-1, 1, (len(g['out_coords']), cout)).astype(np.float32)
    w = rs.uniform(-1, 1, (cout, 3, 3, 3, cin)).astype(np.float32)
    want = ref_grads(g, x, dy, w)
    dw, dx = gpu_grads(g, x, dy, w)
    bound = tr.dw_bound(g['nbr'], want['dw_abs'], cin)
    err = np.abs(dw.astype(np.float64) - want['dw']).reshape(cout, K, cin)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert np.isfinite(dw).all() and (err <= bound).all(), ratio
    ratio_dx = 0.0
    if cin >= 16:
        bdx = (K * cout + 2) * U * want['dx_abs']
        edx = np.abs(dx.astype(np.float64) - want['dx'])
        ratio_dx = float((edx / np.maximum(bdx, 1e-300)).max())
        assert np.isfinite(dx).all() and (edx <= bdx).all(), ratio_dx
    _WORST[(cin, cout, GEOMS.index(geom))] = (ratio, ratio_dx)
    print('spconv train %3d -> %3d %s: largest error / bound  dW %.3f  dx %.3f' % (cin, cout, GEOM_IDS[GEOMS.index(geom)], ratio, ratio_dx))


@pytest.mark.parametrize('chunk', [16, 48])
def test_chunk_boundaries(chunk):
    """the chunk-length argument forced: at least three chunks, the last one partial; equal in the integer case, within the bound in the float one"""
    g = geometry(SUBM)
    n = len(SITES)
    assert n >= 3 * 48 and n % 48 and n % 16
    x, dy, w = int_case(g, 16, 32, 3)
    want = ref_grads(g, x, dy, w)
    dw, _ = gpu_grads(g, x, dy, w, chunk_rows=chunk, want_dx=False)
    assert np.array_equal(dw.astype(np.float64), want['dw'])
    rs = np.random.RandomState(4)
    x, dy, w = (rs.uniform(-1, 1, a.shape).astype(np.float32) for a in (x, dy, w))
    want = ref_grads(g, x, dy, w)
    dw, _ = gpu_grads(g, x, dy, w, chunk_rows=chunk, want_dx=False)
    err = np.abs(dw.astype(np.float64) - want['dw']).reshape(32, 27, 16)
    assert (err <= tr.dw_bound(g['nbr'], want['dw_abs'], 16)).all()
    L = lib.load()
    assert L.pcp_spconv3d_wgrad_workspace_bytes(n, 27, 16, 32, chunk) > L.pcp_spconv3d_wgrad_workspace_bytes(n, 27, 16, 32, 0) > 0
    assert L.pcp_spconv3d_wgrad_workspace_bytes(n, 27, 16, 32, 10) == 0                    # not a multiple of 16


@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65])
def test_row_counts_around_the_tile_sizes(n):
    g = geometry(SUBM, np.ascontiguousarray(SITES[:n]))
    x, dy, w = int_case(g, 16, 32, 50 + n)
    want = ref_grads(g, x, dy, w)
    dw, dx = gpu_grads(g, x, dy, w)
    assert np.array_equal(dw.astype(np.float64), want['dw']) and np.array_equal(dx.astype(np.float64), want['dx'])


def test_no_rows():
    dw = torch.full((32, 3, 3, 3, 16), float('nan'), device='cuda')
    tops.spconv3d_wgrad(torch.zeros((0, 16), device='cuda'), torch.zeros((0, 32), device='cuda'), torch.zeros((27, 0), dtype=torch.int32, device='cuda'),
                        dw)
    assert float(dw.abs().max()) == 0.0
    assert tuple(tops.spconv_invert_nbr(torch.zeros((27, 0), dtype=torch.int32, device='cuda'), 5).shape) == (27, 5)
    assert int(tops.spconv_invert_nbr(torch.zeros((27, 0), dtype=torch.int32, device='cuda'), 5).max()) == -1


def test_repeats_bit_for_bit_and_is_batch_invariant():
    g = geometry(SUBM)
    rs = np.random.RandomState(9)
    x = rs.uniform(-1, 1, (len(SITES), 32)).astype(np.float32)
    dy = rs.uniform(-1, 1, (len(SITES), 64)).astype(np.float32)
    w = rs.uniform(-1, 1, (64, 3, 3, 3, 32)).astype(np.float32)
    dw1, dx1 = gpu_grads(g, x, dy, w)
    dw2, dx2 = gpu_grads(g, x, dy, w)
    assert np.array_equal(dw1.view(np.uint32), dw2.view(np.uint32)) and np.array_equal(dx1.view(np.uint32), dx2.view(np.uint32))
    for b in (0, 2):
        rows = SITES[:, 0] == b
        ga = geometry(SUBM, np.ascontiguousarray(SITES[rows]))
        _, dxa = gpu_grads(ga, x[rows], dy[rows], w)
        assert np.array_equal(dxa.view(np.uint32), dx1[rows].view(np.uint32)), b


def test_dense_backward_is_exact():
    g = geometry(STRIDED[0])
    oc = g['out_coords']
    Bq, D, H, W = (B,) + sr.out_shape(SPATIAL, 3, 2, 1)
    C = 24
    rs = np.random.RandomState(10)
    dcanvas = rs.randn(Bq, H, W, C * D).astype(np.float32)
    want = dcanvas.reshape(Bq, H, W, C, D)[oc[:, 0], oc[:, 2], oc[:, 3], :, oc[:, 1]]
    assert not (oc[:, 0] == 1).any()                                                       # the empty frame
    got = tops.spconv_dense_backward(dev(dcanvas), dev(oc), (Bq, D, H, W), C)
    assert np.array_equal(got.cpu().numpy(), want)
    # and it is the gradient of spconv_dense: sum(dense(f) * dcanvas) differentiates to the same gather
    f = rs.randn(len(oc), C).astype(np.float32)
    table = ops.spconv_table(dev(oc), Bq, (D, H, W))
    dense = ops.spconv_dense(dev(f), table).cpu().numpy()
    assert np.isclose((dense.astype(np.float64) * dcanvas).sum(), (f.astype(np.float64) * want).sum(), rtol=1e-9)


def test_refusals():
    n = len(SITES)
    g = geometry(SUBM)
    nbr, _ = gpu_tables(g)
    x16, dy64 = torch.zeros((n, 16), device='cuda'), torch.zeros((n, 64), device='cuda')
    with pytest.raises(NotImplementedError, match=r'\(16, 64\)'):
        tops.spconv3d_wgrad(x16, dy64, nbr, torch.zeros((64, 3, 3, 3, 16), device='cuda'))
    with pytest.raises(NotImplementedError, match=r'\(32, 16\)'):                          # a data-gradient pair only: no weight gradient
        tops.spconv3d_wgrad(torch.zeros((n, 32), device='cuda'), x16, nbr, torch.zeros((16, 3, 3, 3, 32), device='cuda'))
    with pytest.raises(NotImplementedError, match=r'\(16, 128\)'):
        ops.spconv3d(x16, nbr, torch.zeros((27, 128, 16), device='cuda'), torch.zeros(128, device='cuda'))
    L = lib.load()
    assert L.pcp_spconv3d_wgrad_workspace_bytes(n, 27, 16, 64, 0) == 0
    with pytest.raises(lib.PcpError, match='workspace too small'):
        tops.spconv3d_wgrad(x16, torch.zeros((n, 32), device='cuda'), nbr, torch.zeros((32, 3, 3, 3, 16), device='cuda'),
                            workspace=torch.empty(256, dtype=torch.uint8, device='cuda'))
