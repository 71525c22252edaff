"""The wide stride-2 3x3 direct kernel (k_conv3x3_s2w, option conv_s2_form = 2) against the form it replaces (k_conv3x3<2, 8, 8, 64, 2, 2>,
conv_s2_form = 1) -- bit for bit, since it keeps every output's summation order -- and against float64 conv2d on the CPU within 2e-4 of
the output scale (the bar DESIGN.md gives the fp32 conv tests).  Run on the GPU box:  python -m pytest tests/test_gpu_conv_s2.py -m gpu -q
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pcp_amd import synth

pytestmark = pytest.mark.gpu

MAPS = [(1, 16, 16), (2, 17, 23), (1, 33, 9), (1, 40, 72)]      # whole tiles | odd (last row / column, right and bottom halo) | narrower than a tile | several tiles
CINS = [16, 64]                                                   # one slice | several (the double buffer and the weight ring wrap)
COUTS = [64, 128, 192, 100]                                       # 64-tile | 128-tile | cout_pad % 128 != 0: three 64-tiles | padded channels
PAD_IN, OFF_IN, PAD_OUT, OFF_OUT = 16, 8, 24, 8                   # the wide buffers: ld_in = cin + 16 read from channel 8, ld_out = cout + 24 written at 8
FILL = 7.0


def dev():
    assert torch.cuda.is_available(), 'gpu-marked tests need the MI355X'
    return torch.device('cuda:0')


def _rand(seed, shape, lo=-1.0, hi=1.0):
    return synth.uniform(seed, 5, int(np.prod(shape)), lo, hi).reshape(shape)


@functools.lru_cache(maxsize=None)
def _case(bhw, cin, cout):
    """inputs (the activations inside a wider buffer), packed weights and the float64 reference without ReLU; computed once per case"""
    from pcp_amd import pack
    B, H, W = bhw
    xw = torch.from_numpy(_rand(11, (B, H, W, cin + PAD_IN)))
    wt = torch.from_numpy(_rand(12, (cout, cin, 3, 3), -0.05, 0.05))
    b = torch.from_numpy(_rand(13, (cout,), -0.2, 0.2))
    x = xw[..., OFF_IN:OFF_IN + cin]
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    packed, bp, cpad = pack.pack_conv3x3(wt, b)
    return xw, x.contiguous(), packed, bp, cpad, want


def _run(lib_option, form, x, packed, bp, cin, cout, cpad, relu, out=None, in_ch_off=0, out_ch_off=0):
    from pcp_amd import ops
    lib_option('conv_s2_form', form)
    got = ops.conv3x3(x, packed, bp, cin, cout, cpad, stride=2, relu=relu, out=out, in_ch_off=in_ch_off, out_ch_off=out_ch_off)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('cin', CINS)
@pytest.mark.parametrize('bhw', MAPS)
def test_wide_form_equals_old_form_bitwise(lib_option, bhw, cin, cout):
    d = dev()
    xw, x, packed, bp, cpad, _ = _case(bhw, cin, cout)
    xw, x, packed, bp = xw.to(d), x.to(d), packed.to(d), bp.to(d)
    B, H, W = bhw
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for relu in (True, False):
        old = _run(lib_option, 1, x, packed, bp, cin, cout, cpad, relu)
        new = _run(lib_option, 2, x, packed, bp, cin, cout, cpad, relu)
        assert old.shape == (B, ho, wo, cout) and torch.equal(old, new), (relu, float((old - new).abs().max()))
        # inside wider buffers: the same bits in the written columns, the fill everywhere else
        outs = []
        for form in (1, 2):
            out = torch.full((B, ho, wo, cout + PAD_OUT), FILL, device=d)
            _run(lib_option, form, xw, packed, bp, cin, cout, cpad, relu, out=out, in_ch_off=OFF_IN, out_ch_off=OFF_OUT)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[1][..., OFF_OUT:OFF_OUT + cout], new)
        assert bool((outs[1][..., :OFF_OUT] == FILL).all()) and bool((outs[1][..., OFF_OUT + cout:] == FILL).all())


@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('cin', CINS)
@pytest.mark.parametrize('bhw', MAPS)
def test_wide_form_matches_float64_conv2d(lib_option, bhw, cin, cout):
    d = dev()
    xw, x, packed, bp, cpad, want = _case(bhw, cin, cout)
    xw, packed, bp = xw.to(d), packed.to(d), bp.to(d)
    B, H, W = bhw
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for relu in (True, False):
        ref = F.relu(want) if relu else want
        scale = float(ref.abs().max())
        out = torch.full((B, ho, wo, cout + PAD_OUT), FILL, device=d)
        _run(lib_option, 2, xw, packed, bp, cin, cout, cpad, relu, out=out, in_ch_off=OFF_IN, out_ch_off=OFF_OUT)
        err = float((out[..., OFF_OUT:OFF_OUT + cout].cpu().double() - ref).abs().max())
        print('%s cin %d cout %d relu %d: max err %.3g of scale %.3g' % (bhw, cin, cout, relu, err, scale))
        assert err <= 2e-4 * scale, (err, scale)


@pytest.mark.parametrize('cout', [128, 100])
def test_wide_form_unaligned_output_rows(lib_option, cout):
    """ld_out % 4 != 0: no 16-byte stores; the columns around the written ones keep their fill"""
    d = dev()
    bhw, cin = (2, 17, 23), 64
    _, x, packed, bp, cpad, want = _case(bhw, cin, cout)
    x, packed, bp = x.to(d), packed.to(d), bp.to(d)
    B, ho, wo = 2, 9, 12
    outs = []
    for form in (1, 2):
        out = torch.full((B, ho, wo, cout + 3), FILL, device=d)
        _run(lib_option, form, x, packed, bp, cin, cout, cpad, True, out=out, out_ch_off=1)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[1][..., :1] == FILL).all()) and bool((outs[1][..., 1 + cout:] == FILL).all())
    ref = F.relu(want)
    err = float((outs[1][..., 1:1 + cout].cpu().double() - ref).abs().max())
    assert err <= 2e-4 * float(ref.abs().max()), err


def test_rule_is_the_wide_form_and_bad_values_are_refused(lib_option):
    """no override: the built-in rule; its bits are those of both forms.  Values other than 0, 1, 2 are an argument error at the launch"""
    from pcp_amd import lib
    d = dev()
    bhw, cin, cout = (1, 40, 72), 64, 128
    _, x, packed, bp, cpad, _ = _case(bhw, cin, cout)
    x, packed, bp = x.to(d), packed.to(d), bp.to(d)
    rule = _run(lib_option, None, x, packed, bp, cin, cout, cpad, True)
    assert torch.equal(rule, _run(lib_option, 1, x, packed, bp, cin, cout, cpad, True))
    with pytest.raises(lib.PcpError):
        _run(lib_option, 3, x, packed, bp, cin, cout, cpad, True)
