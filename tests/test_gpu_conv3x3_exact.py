"""The fp32 3x3 forward convolutions against the float64 references of tests/conv3x3_refs.py: k_conv3x3 (strides 1 and 2, both values of
conv_s2_form), k_wino, the wave-stationary F(2x2) kernel, through-memory F(4x4), the fused k_wino4f / k_wino4h / k_wino4c (wino4c_nw 4
and 8) and the bf16x3 split, called through the pcp_amd.ops wrappers with weights from the matching pack.pack_conv3x3_*.

Integer cases: inputs on which every correct fp32 evaluation gives the same bits whatever its tiling or k order (conv3x3_refs' docstring
has the proof and tests/test_conv3x3_refs_cpu.py the condition); the kernels owe the float64 result exactly, twice.  They see every
indexing, padding, packing and ordering mistake and are blind to lost precision.  Float cases: the same shapes on uniform data; the error
against float64 stays below a derived, element-wise bar: bound(S, 9 cin + 1) for the direct kernels, bound(T, cin + 16) with the Winograd
scale T for the Winograd kernels, the direct bar plus the residual of the three-term split for bf16x3.  Channel-window cases: one per
kernel, integer data read at a channel offset of a wider buffer and written into a wider buffer that keeps its fill elsewhere.

Largest err / bar per kernel on the MI355X (each test prints its own):
  direct, stride 1                0.030        F(2x2) k_wino                  0.022        fused F(4x4) k_wino4f               0.012
  direct, stride 2, form 1 and 2  0.026        F(2x2) wave-stationary         0.011        fused F(4x4) k_wino4h               0.011
  bf16x3, stride 1                0.141        F(4x4) through memory          0.004        fused F(4x4) k_wino4c, nw 4 and 8   0.011
  bf16x3, stride 2                0.096
Every integer case was bit-equal.  By hand, on a scratch copy: weights packed with kx mirrored, or with the last eight-channel slice of U
zeroed, fail every integer and every float case of k_wino4c.

Run on the GPU box:  python -m pytest tests/test_gpu_conv3x3_exact.py -m gpu -q -s
"""
import functools

import numpy as np
import pytest
import torch

import conv3x3_refs as cr

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'gpu-marked tests need the MI355X'
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _packed(pack_name, table, i, variant):
    """(packed weights, padded bias, cout_pad) on the CPU, once per pack function and case"""
    from pcp_amd import pack
    d = cr.case_data(table, i, variant)
    return getattr(pack, pack_name)(torch.from_numpy(np.array(d['w'])), torch.from_numpy(np.array(d['b'])))


def _launch(name, i, variant, relu, lib_option, x=None, out=None, in_ch_off=0, out_ch_off=0):
    """one launch of kernel `name` on case i: the output tensor"""
    from pcp_amd import ops
    k = cr.KERNELS[name]
    c = cr.TABLES[k.table][i]
    packed, bias, cpad = _packed(k.pack, k.table, i, variant)
    if k.option:
        lib_option(*k.option)
    d = dev()
    if x is None:
        x = torch.from_numpy(np.array(cr.case_data(k.table, i, variant)['x']))
    kw = dict(relu=relu, out=out, in_ch_off=in_ch_off, out_ch_off=out_ch_off)
    if k.algo in ('direct', 'bf16x3'):
        kw['stride'] = c.stride
    got = getattr(ops, k.op)(x.to(d), packed.to(d), bias.to(d), c.cin, c.cout, cpad, **kw)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('name,i', cr.KERNEL_CASES)
def test_integer_cases_are_bit_equal_to_float64(name, i, lib_option):
    k = cr.KERNELS[name]
    pre = cr.case_data(k.table, i, 'ints')['pre']
    for relu in (False, True):
        want = (np.maximum(pre, 0.0) if relu else pre).astype(np.float32)
        got = _launch(name, i, 'ints', relu, lib_option)
        again = _launch(name, i, 'ints', relu, lib_option)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))                          # the same bits twice
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.any()
        wrong = got != want                                                                         # numerically: -0 equals +0
        assert not wrong.any(), '%s %s relu %d: %d of %d elements differ, first at %s: got %r want %r' % (
            name, cr.TABLES[k.table][i], relu, wrong.sum(), wrong.size, np.argwhere(wrong)[0], got[wrong][0], want[wrong][0])


@pytest.mark.parametrize('name,i', cr.KERNEL_CASES)
def test_float_cases_stay_inside_the_derived_bar(name, i, lib_option):
    k = cr.KERNELS[name]
    d = cr.case_data(k.table, i, 'float')
    for relu in (False, True):
        want = np.maximum(d['pre'], 0.0) if relu else d['pre']
        got = _launch(name, i, 'float', relu, lib_option).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        ratio = np.abs(got - want) / d['bar']
        print('RATIO %s case %d relu %d: largest err / bar %.4f' % (name, i, relu, ratio.max()))
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1.0, '%s %s relu %d: err / bar %.3f at %s (got %r want %r bar %.3e)' % (
            name, cr.TABLES[k.table][i], relu, ratio.max(), at, got[at], want[at], d['bar'][at])


@pytest.mark.parametrize('name', sorted(cr.WINDOW_CASE))
def test_channel_windows_are_exact_and_leave_the_fill(name, lib_option):
    k = cr.KERNELS[name]
    i = cr.WINDOW_CASE[name]
    c = cr.TABLES[k.table][i]
    d = cr.case_data(k.table, i, 'ints')
    Ho, Wo = cr.out_hw(c.H, c.W, c.stride)
    wide = cr.ints8(7000 + i, 1, (c.B, c.H, c.W, c.cin + cr.PAD_IN))                                 # what a kernel that ignores the window reads
    wide[..., cr.OFF_IN:cr.OFF_IN + c.cin] = d['x']
    for relu in (False, True):
        want = (np.maximum(d['pre'], 0.0) if relu else d['pre']).astype(np.float32)
        out = torch.full((c.B, Ho, Wo, c.cout + cr.PAD_OUT), cr.FILL, device=dev())
        _launch(name, i, 'ints', relu, lib_option, x=torch.from_numpy(wide), out=out, in_ch_off=cr.OFF_IN, out_ch_off=cr.OFF_OUT)
        got = out.cpu().numpy()
        assert np.array_equal(got[..., cr.OFF_OUT:cr.OFF_OUT + c.cout], want) and got[..., cr.OFF_OUT:cr.OFF_OUT + c.cout].any()
        assert (got[..., :cr.OFF_OUT] == cr.FILL).all() and (got[..., cr.OFF_OUT + c.cout:] == cr.FILL).all()
