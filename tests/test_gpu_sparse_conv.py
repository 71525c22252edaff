"""The sparse first backbone layer (k_sparse_conv_s2 through pcp_sparse_conv3x3_s2 / pcp_mp_sparse_conv3x3_s2) against the float64
reference of tests/sparse_conv_refs.py, on the occupancy patterns of its case table: non-square and odd grids, partial tiles, and per
(tile, tap) row counts placed on every branch point of the kernel (tests/test_sparse_conv_refs_cpu.py asserts which).

Every case pillarises the points of its pattern, checks that the pillar list IS the pattern, and hands the kernel pillar rows whose tail
past P is NaN.  Integer cases: data on which every correct fp32 evaluation gives the same bits in any order; the kernel owes the float64
result exactly, twice, with ReLU off and on.  Float cases: the same shapes on uniform data; |got - ref| <= bound(S, 9 * 64 + 9 + 1) element
by element.  One-hot weights turn the layer into a lookup of pillar rows, which pins the tap geometry and the order of the cell table
without any sum.  Further: every cout % 4 == 0 width class, wider output rows that keep their fill, bf16 output (nearest even, ties
included), the workspaces of the other pillarisers, empty clouds, and the documented refusals, which launch nothing.

On the MI355X every integer case was bit-equal and the largest err / bar of the float cases was 0.0066 (case whole_63_64_65, ReLU off;
every case prints its own).  A recorded observation, not a threshold.

By hand, on a scratch copy of csrc/sparseconv.hip, one line broken at a time, the integer cases that fail:
  cell table read as iy * nx + ix             28 of the 31 cases, the first wide_full; every one-hot case.  wide_empty, one_cell and
                                              wide_single_corner pass: no cell, one cell, and the last cell, whose index is the same
                                              either way
  second row tile run only at 32 rows         tall_17_31_33 (and 19 more: every case with a chunk of 17..31 rows); wide_edge_tile_15_16
  (rows_i >= 32 * rtile)                      and whole_1_32_128 pass, as they must
  second tail stage dropped                   wide_items_5_6_7, whole_63_64_65, whole_96_97_127 (tiles of 3 or 7 items) and eight more
  staged rows stored without the              none, and none can: a staged row past the chunk only reaches the same row of the product
  g_row < rows_i select                       block, which the pixel mask (pixs = -1) never adds anywhere.  The select is no part of what
                                              the layer computes; the rows past P that a kernel must not multiply are the NaN tail here

Run on the GPU box:  python -m pytest tests/test_gpu_sparse_conv.py -m gpu -q -s
"""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_refs as sr

pytestmark = pytest.mark.gpu

ALL = list(range(len(sr.CASES)))
IDS = [c.name for c in sr.CASES]
TAIL = 64                                    # rows of NaN behind the P pillar rows


def dev():
    assert torch.cuda.is_available(), 'gpu-marked tests need the MI355X'
    return torch.device('cuda:0')


def _grid(c):
    from pcp_amd import ops
    g = sr.grid_of(c)
    return ops.make_grid(sr.pc_range(g), sr.voxel_size(g), sr.grid_size(g), c.B)


def _pillarise(c, pts=None, rows=None, bucket_order=False):
    """the case's points through pcp_voxelize (or, rows = num_raw, pcp_pillarise_rows): (VoxelizeResult, voxel_coords[:P] as numpy), after
    the precondition that the pillar list is the case's occupancy, each cell once"""
    from pcp_amd import ops
    occ = sr.occupancy(c)
    if pts is None:
        pts = sr.points_for(occ, sr.grid_of(c))
    if rows is not None and pts.shape[1] < rows + 1:                          # the raw columns 1 .. num_raw must exist
        pts = np.concatenate([pts, np.full((pts.shape[0], rows + 1 - pts.shape[1]), 0.25, np.float32)], 1)
    pd = torch.from_numpy(np.ascontiguousarray(pts)).to(dev())
    if rows is None:
        vox = ops.voxelize(pd, _grid(c), want_inverse=False, want_counts=False)
    else:
        vox = ops.pillarise_rows(pd, _grid(c), rows, want_coords=True, bucket_order=bucket_order)
    P = int(vox.counters[0])
    vc = vox.voxel_coords[:P].cpu().numpy()
    return vox, vc


def _check_pillars(occ, vc):
    seen = np.zeros_like(occ)
    seen[vc[:, 0], vc[:, 2], vc[:, 3]] = True
    assert vc.shape[0] == int(occ.sum()) and np.array_equal(seen, occ) and not vc[:, 1].any(), 'the pillar list is not the pattern'


def _rows(pf):
    """(P + TAIL, 64) on the device: pf in front, NaN behind"""
    t = torch.full((pf.shape[0] + TAIL, 64), float('nan'), device=dev())
    if pf.shape[0]:
        t[:pf.shape[0]] = torch.from_numpy(np.array(pf)).to(dev())
    return t


def _launch(vox, pf, w, b, relu, out=None, out_dtype=torch.float32):
    from pcp_amd import ops, pack
    wp, bp = pack.pack_conv3x3_sparse_s2(torch.from_numpy(np.array(w)), torch.from_numpy(np.array(b)))
    got = ops.sparse_conv3x3_s2(_rows(pf), vox, wp.to(dev()), bp.to(dev()), w.shape[0], relu=relu, out=out, out_dtype=out_dtype)
    torch.cuda.synchronize()
    return got


def _case(i, variant, cout=None, rows=None, bucket_order=False):
    """pillarise CASES[i] and pair it with its cached inputs: (vox, data dict whose pre / S belong to THIS call's pillar order)"""
    c = sr.CASES[i]
    d = sr.case_data(i, variant, cout)
    vox, vc = _pillarise(c, rows=rows, bucket_order=bucket_order)
    _check_pillars(d['occ'], vc)
    if not np.array_equal(vc, d['coords']):                                    # another pillar order: row p sits in another cell
        pre, S = sr.reference(d['occ'], vc, d['pf'], d['w'], d['b'], False)
        d = dict(d, coords=vc, pre=pre, S=S, bar=None if d['bar'] is None else sr.bound(S, sr.BAR_K))
    return vox, d


def _want(pre, relu):
    return (np.maximum(pre, 0.0) if relu else pre).astype(np.float32)


def _assert_bits(got, want, what):
    assert got.shape == want.shape and not np.isnan(got).any(), what
    wrong = got != want                                                        # numerically: -0 equals +0
    assert not wrong.any(), '%s: %d of %d elements differ, first at %s: got %r want %r' % (
        what, wrong.sum(), wrong.size, np.argwhere(wrong)[0], got[wrong][0], want[wrong][0])


# ---- 1, 2: every case, integer and float ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i', ALL, ids=IDS)
def test_integer_cases_are_bit_equal_to_float64(i):
    vox, d = _case(i, 'ints')
    for relu in (False, True):
        got = _launch(vox, d['pf'], d['w'], d['b'], relu)
        again = _launch(vox, d['pf'], d['w'], d['b'], relu)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))                          # the same bits twice
        got = got.cpu().numpy()
        assert got.any()
        _assert_bits(got, _want(d['pre'], relu), '%s relu %d' % (sr.CASES[i].name, relu))


@pytest.mark.parametrize('i', ALL, ids=IDS)
def test_float_cases_stay_inside_the_derived_bar(i):
    vox, d = _case(i, 'float')
    for relu in (False, True):
        want = np.maximum(d['pre'], 0.0) if relu else d['pre']
        got = _launch(vox, d['pf'], d['w'], d['b'], relu).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and not np.isnan(got).any()
        ratio = np.abs(got - want) / d['bar']
        print('RATIO %s relu %d: largest err / bar %.4f' % (sr.CASES[i].name, relu, ratio.max()))
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1.0, '%s relu %d: err / bar %.3f at %s (got %r want %r bar %.3e)' % (
            sr.CASES[i].name, relu, ratio.max(), at, got[at], want[at], d['bar'][at])


# ---- 3: one-hot weights -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sr.ONE_HOT_CASES)
def test_one_hot_weights_copy_the_pillar_row_of_the_tapped_cell(name):
    vox, d = _case(sr.CASE_INDEX[name], 'float')
    for tap in range(9):
        got = _launch(vox, d['pf'], sr.one_hot_weights(tap), np.zeros(64, np.float32), False).cpu().numpy()
        want = sr.one_hot_expect(d['occ'], d['coords'], d['pf'], tap)
        assert want.any()
        _assert_bits(got, want, '%s tap %d' % (name, tap))


# ---- 4: output widths -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cout', sr.COUTS)
def test_every_output_width_is_bit_equal(cout):
    vox, d = _case(sr.CASE_INDEX[sr.COUT_CASE], 'ints', cout)
    for relu in (False, True):
        got = _launch(vox, d['pf'], d['w'], d['b'], relu).cpu().numpy()
        assert got.shape[-1] == cout
        _assert_bits(got, _want(d['pre'], relu), 'cout %d relu %d' % (cout, relu))


# ---- 5: wider output rows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cout', sr.WIDE_ROW_COUTS)
def test_wider_output_rows_keep_their_fill(cout):
    i = sr.CASE_INDEX[sr.WIDE_ROW_CASE]
    c = sr.CASES[i]
    vox, d = _case(i, 'ints', cout)
    ho, wo = sr.out_hw(c.ny, c.nx, 2)
    for relu in (False, True):
        out = torch.full((c.B, ho, wo, cout + sr.WIDE_ROW_PAD), sr.FILL, device=dev())
        _launch(vox, d['pf'], d['w'], d['b'], relu, out=out)
        got = out.cpu().numpy()
        _assert_bits(got[..., :cout], _want(d['pre'], relu), 'cout %d of ld_out %d relu %d' % (cout, cout + sr.WIDE_ROW_PAD, relu))
        assert (got[..., cout:] == sr.FILL).all()


# ---- 6: bf16 output ---------------------------------------------------------------------------------------------------------------------

def _bf16(a32):
    return torch.from_numpy(np.ascontiguousarray(a32)).to(torch.bfloat16)


@pytest.mark.parametrize('name', sr.BF16_CASES)
def test_bf16_output_is_the_reference_rounded_to_nearest_even(name):
    vox, d = _case(sr.CASE_INDEX[name], 'ints')
    assert (np.abs(d['pre']) > 256).any()
    for relu in (False, True):
        got = _launch(vox, d['pf'], d['w'], d['b'], relu, out_dtype=torch.bfloat16)
        assert got.dtype == torch.bfloat16
        want = _bf16(_want(d['pre'], relu))
        g, w = got.cpu().float().numpy(), want.float().numpy()
        _assert_bits(g, w, '%s bf16 relu %d' % (name, relu))


def test_wider_bf16_rows_keep_their_fill():
    i = sr.CASE_INDEX[sr.WIDE_ROW_CASE]
    c = sr.CASES[i]
    cout = sr.WIDE_ROW_COUTS[0]
    vox, d = _case(i, 'ints', cout)
    ho, wo = sr.out_hw(c.ny, c.nx, 2)
    for relu in (False, True):
        out = torch.full((c.B, ho, wo, cout + sr.WIDE_ROW_PAD), sr.FILL, device=dev(), dtype=torch.bfloat16)
        _launch(vox, d['pf'], d['w'], d['b'], relu, out=out)
        got = out.cpu().float().numpy()
        _assert_bits(got[..., :cout], _bf16(_want(d['pre'], relu)).float().numpy(), 'bf16 cout %d relu %d' % (cout, relu))
        assert (got[..., cout:] == sr.FILL).all()


# ---- 7: the other pillarisers' workspaces -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num_raw,bucket_order', [(4, False), (5, False), (5, True)])
def test_rows_pillariser_workspaces_give_the_same_layer(num_raw, bucket_order):
    vox, d = _case(sr.CASE_INDEX[sr.OTHER_PILLARISER_CASE], 'ints', rows=num_raw, bucket_order=bucket_order)
    for relu in (False, True):
        got = _launch(vox, d['pf'], d['w'], d['b'], relu).cpu().numpy()
        _assert_bits(got, _want(d['pre'], relu), 'pillarise_rows num_raw %d bucket_order %d relu %d' % (num_raw, bucket_order, relu))


# ---- 8: no pillars ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cloud', ['no_rows', 'all_outside'])
def test_a_cloud_without_pillars_gives_the_bias(cloud):
    i = sr.CASE_INDEX['wide_empty']
    c = sr.CASES[i]
    d = sr.case_data(i, 'ints')
    pts = np.zeros((0, 5), np.float32)
    if cloud == 'all_outside':                     # past the far edges, below the origin, a frame that does not exist
        pts = np.array([[0, c.nx * sr.VOXEL + 0.125, 1.125, 0, 0], [1, 1.125, c.ny * sr.VOXEL + 0.125, 0, 0], [0, -0.125, 1.125, 0, 0],
                        [1, 1.125, -0.125, 0, 0], [c.B, 1.125, 1.125, 0, 0], [0, 1e9, 1e9, 0, 0]], np.float32)
    vox, vc = _pillarise(c, pts=pts)
    assert vc.shape[0] == 0
    for relu in (False, True):
        got = _launch(vox, d['pf'], d['w'], d['b'], relu).cpu().numpy()
        want = np.broadcast_to(np.maximum(d['b'], 0) if relu else d['b'], got.shape)
        _assert_bits(got, want, '%s relu %d' % (cloud, relu))
        _assert_bits(got, _want(d['pre'], relu), '%s relu %d against the reference' % (cloud, relu))


# ---- 9: documented refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_return_their_code_and_leave_the_output_alone():
    """sparse_conv_impl's checks, in its order: ARG for a missing pointer, UNSUPPORTED for a width it has no kernel for, ARG for a pointer
    that is not 16-byte aligned; the mp entry ARG for a storage type it does not know.  All of them before any launch"""
    from pcp_amd import lib, ops, pack
    L = lib.load()
    i = sr.CASE_INDEX['odd_density_05']
    c = sr.CASES[i]
    vox, d = _case(i, 'ints')
    ho, wo = sr.out_hw(c.ny, c.nx, 2)
    wp, bp = pack.pack_conv3x3_sparse_s2(torch.from_numpy(np.array(d['w'])), torch.from_numpy(np.array(d['b'])))
    # every buffer with room behind it, so that an offset pointer still points into it
    pf = torch.cat([_rows(d['pf']).reshape(-1), torch.zeros(4, device=dev())])
    wp = torch.cat([wp.reshape(-1), torch.zeros(4)]).to(dev())
    bp = torch.cat([bp, torch.zeros(4)]).to(dev())
    out = torch.full((c.B * ho * wo * 64 + 4,), sr.FILL, device=dev())
    base = dict(pf=pf.data_ptr(), w=wp.data_ptr(), b=bp.data_ptr(), out=out.data_ptr(), cout=64, ld=64)

    def call(mp_dtype=None, refused=True, **kw):
        a = dict(base, **kw)
        front = (ctypes.c_void_p(a['pf']), ctypes.byref(vox.grid), ctypes.c_void_p(vox.workspace.data_ptr()), vox.n, ctypes.c_void_p(a['w']),
                 ctypes.c_void_p(a['b']), a['cout'], 0, ctypes.c_void_p(a['out']))
        stream = ctypes.c_void_p(ops.current_stream_handle())
        if mp_dtype is None:
            st = L.pcp_sparse_conv3x3_s2(*front, a['ld'], stream)
        else:
            st = L.pcp_mp_sparse_conv3x3_s2(*front, mp_dtype, a['ld'], stream)
        torch.cuda.synchronize()
        if refused:
            assert bool((out == sr.FILL).all()), 'a refused call wrote to the output: %r' % (kw,)
        return st

    for cout in (0, 6, 68):
        assert call(cout=cout, ld=72) == lib.ERR_UNSUPPORTED, cout
    assert call(cout=64, ld=60) == lib.ERR_UNSUPPORTED                       # ld_out < cout
    assert call(cout=32, ld=34) == lib.ERR_UNSUPPORTED                       # ld_out % 4
    for which in ('pf', 'w', 'b', 'out'):
        assert call(**{which: base[which] + 4}) == lib.ERR_ARG, which
        assert call(mp_dtype=lib.DT_F32, **{which: base[which] + 4}) == lib.ERR_ARG, which
    assert call(mp_dtype=lib.DT_BF16, out=base['out'] + 4) == lib.ERR_ARG    # bf16 rows want 8 bytes
    assert call(mp_dtype=2) == lib.ERR_ARG
    # and the same arguments without a fault run
    assert call(refused=False) == lib.OK
    got = out[:-4].view(c.B, ho, wo, 64).cpu().numpy()
    _assert_bits(got, _want(d['pre'], False), 'the accepted call')
