"""Shared plumbing for the dense conv stacks: turns (Conv2d | ConvTranspose2d) [+ BatchNorm2d] parameter containers into
packed HIP weights and launches them on NHWC buffers."""
import torch
import torch.nn as nn

from pcp_amd import lib, ops, pack
from pcp_amd.conv_dispatch import Forms, choose_conv3x3, conv_algo, forms_for


def _plain_bf16():
    return conv_algo() == 'bf16'


_PW_MODE = {'plain': lib.PW_PLAIN, 's2d': lib.PW_SPACE2DEPTH, 'd2s': lib.PW_DEPTH2SPACE}
# kernel name of conv_dispatch.choose_conv3x3 -> (slot of the packed form, function of pcp_amd.ops).  The function is looked up on the module
# at every call: tests and the bench tools replace ops.conv3x3_* by name
_LAUNCH = {'direct': ('w', 'conv3x3'), 'winograd': ('wino', 'conv3x3_winograd'), 'winograd4': ('w4', 'conv3x3_winograd4'),
           'winograd4f': ('w4f', 'conv3x3_winograd4f'), 'winograd4h': ('w4h', 'conv3x3_winograd4h'),
           'winograd4c': ('w4c', 'conv3x3_winograd4c'), 'bf16x3': ('b3', 'conv3x3_bf16x3')}
_REPACK = {'w4h': pack.repack_winograd4f_to_4h, 'w4c': pack.repack_winograd4f_to_4c}       # forms made from w4f at their first launch


class PackedConv:
    """One fused conv(+BN)(+ReLU) launch description.  packed: the (weights, bias, cout_pad) of the direct / pointwise kernel; the other
    slots hold the same triple for the other 3x3 kernels, None where the layer has no such form (conv_dispatch.forms_for)."""
    __slots__ = ('kind', 'w', 'b', 'cin', 'cout', 'cout_pad', 'stride', 'relu', 'wino', 'b3', 'w4', 'w4f', 'w4h', 'w4c', 'mp')

    def __init__(self, kind, cin, cout, relu, packed, stride=1):
        self.kind, self.cin, self.cout, self.relu, self.stride = kind, cin, cout, relu, stride
        self.w, self.b, self.cout_pad = packed
        self.wino = self.b3 = self.w4 = self.w4f = self.w4h = self.w4c = self.mp = None

    def _form(self, slot):
        if slot == 'w':
            return self.w, self.b, self.cout_pad
        if slot in _REPACK and getattr(self, slot) is None:
            setattr(self, slot, (_REPACK[slot](self.w4f[0]), self.w4f[1], self.w4f[2]))
        return getattr(self, slot)

    def run(self, x, out=None, in_ch_off=0, out_ch_off=0):
        if self.kind != '3x3':
            return self._run_pointwise(x, out, in_ch_off, out_ch_off)
        algo = conv_algo()
        B, H, W, ld_in = x.shape
        forms = Forms(*[f and f[2] for f in (self.wino, self.b3, self.w4, self.w4f, self.mp)])
        name = choose_conv3x3(algo, self.cin, self.cout, self.stride, forms, B, H, W, ld_in, in_ch_off,
                              None if out is None else out.shape[-1], out_ch_off, x.dtype == torch.float32)
        if name == 'mp':
            # the bf16 loop of config 5 (include/pcp_hip_mp.h): frozen teachers inside a training iteration run the bf16 kernels on bf16
            # activations -- BatchNorm folded into the bf16 weights + fp32 bias; an fp32 input (the sparse first layer's output, a canvas)
            # is cast once, the output is bf16 unless the caller's buffer says float32
            from pcp_amd import train_ops as tops
            if x.dtype != torch.bfloat16 or in_ch_off % 8 or x.shape[-1] % 8:
                x, in_ch_off = x[..., in_ch_off:in_ch_off + self.cin].to(torch.bfloat16).contiguous(), 0
            wp, bp, cp = self.mp
            return tops.mp_conv3x3(x, wp, bp, self.cin, self.cout, cp, stride=self.stride, relu=self.relu, out=out, in_ch_off=in_ch_off,
                                   out_ch_off=out_ch_off)
        if x.dtype != torch.float32:
            x, in_ch_off = x[..., in_ch_off:in_ch_off + self.cin].float().contiguous(), 0      # the fp32 kernels' view of a bf16 activation
        slot, fn = _LAUNCH[name]
        u, ub, ucp = self._form(slot)
        extra = {}
        if name in ('direct', 'bf16x3'):                   # the two kernels that also take stride 2
            extra['stride'] = self.stride
        if name == 'bf16x3':
            extra['plain'] = algo == 'bf16'
        return getattr(ops, fn)(x, u, ub, self.cin, self.cout, ucp, relu=self.relu, out=out, in_ch_off=in_ch_off, out_ch_off=out_ch_off, **extra)

    def _run_pointwise(self, x, out, in_ch_off, out_ch_off):
        if (self.mp is not None and _plain_bf16() and x.dtype == torch.bfloat16 and in_ch_off % 8 == 0
                and x.shape[-1] % 8 == 0 and (out is None or (out.shape[-1] % 8 == 0 and out_ch_off % 8 == 0))):
            # bf16 loop: a pointwise layer behind a bf16 3x3 layer reads the bf16 map as it lies (pcp_mp_pointwise); its output takes the
            # storage type of the caller's buffer (float32 when it allocates here: the consumers outside the conv stacks are fp32 kernels)
            from pcp_amd import train_ops as tops
            wp, bp, cp = self.mp
            return tops.mp_pointwise(x, wp, bp, _PW_MODE[self.kind], self.cin, self.cout, cp, relu=self.relu, out=out, in_ch_off=in_ch_off,
                                     out_ch_off=out_ch_off, out_dtype=torch.float32)
        if x.dtype != torch.float32:
            x, in_ch_off = x[..., in_ch_off:in_ch_off + self.cin].float().contiguous(), 0      # the fp32 kernels' view of a bf16 activation
        return ops.pointwise(x, self.w, self.b, _PW_MODE[self.kind], self.cin, self.cout, self.cout_pad, relu=self.relu, out=out,
                             in_ch_off=in_ch_off, out_ch_off=out_ch_off)


def _fold(conv, bn, out_axis):
    w = conv.weight.detach().float()
    cb = conv.bias.detach().float() if conv.bias is not None else None
    if bn is None:
        n_out = w.shape[out_axis]
        return w, (cb if cb is not None else torch.zeros(n_out, dtype=torch.float32, device=w.device))
    return pack.fold_bn(w, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, conv_bias=cb,
                        out_axis=out_axis)


def _pack_mp(w, b):
    """(folded) fp32 weights -> the bf16 form of pcp_mp_conv3x3 + padded fp32 bias"""
    from pcp_amd import train_ops as tops
    wp, opad = tops.mp_pack_conv3x3(w.contiguous().float())
    bp = torch.zeros(opad, dtype=torch.float32, device=w.device)
    bp[:b.numel()] = b
    return wp, bp, opad


def _pack_mp_pointwise(pc):
    """bf16 copy of a pointwise layer's packed weights for pcp_mp_pointwise (PCP_CONV_ALGO=bf16 only, shapes the kernel takes)"""
    if conv_algo() == 'bf16' and pc.w.is_cuda and pc.cin % 32 == 0 and pc.cout % 8 == 0 and pc.cout_pad % 64 == 0:
        pc.mp = (pc.w.to(torch.bfloat16).contiguous(), pc.b, pc.cout_pad)


def _pack_conv3x3(w, b, relu, stride):
    """a 3x3 layer with every weight form conv_dispatch.forms_for gives it under the current PCP_CONV_ALGO"""
    pc = PackedConv('3x3', w.shape[1], w.shape[0], relu, pack.pack_conv3x3(w, b), stride=stride)
    forms = forms_for(pc.cin, pc.cout, stride, conv_algo())
    if 'wino' in forms:
        pc.wino = pack.pack_conv3x3_winograd(w, b)
    if 'b3' in forms:
        pc.b3 = pack.pack_conv3x3_bf16x3(w, b)
    if 'mp' in forms and w.is_cuda:
        pc.mp = _pack_mp(w, b)
    if 'w4' in forms:
        pc.w4 = pack.pack_conv3x3_winograd4(w, b)
    if 'w4f' in forms:
        pc.w4f = pack.pack_conv3x3_winograd4f(w, b)
    return pc


# (ConvTranspose2d?, kernel size, stride) -> (kind, packer) of the layers pcp_pointwise runs
_POINTWISE = {(False, 1, 1): ('plain', pack.pack_plain), (False, 2, 2): ('s2d', pack.pack_conv2x2_s2),
              (True, 1, 1): ('plain', pack.pack_convT1x1), (True, 2, 2): ('d2s', pack.pack_convT2x2_s2)}


def pack_conv_module(conv, bn=None, relu=True):
    """conv: nn.Conv2d (3x3 s1/s2 p1 | 1x1 | k2 s2) or nn.ConvTranspose2d (k1 s1 | k2 s2)."""
    transposed = isinstance(conv, nn.ConvTranspose2d)
    w, b = _fold(conv, bn, out_axis=1 if transposed else 0)
    k, s = conv.kernel_size[0], conv.stride[0]
    if not transposed and k == 3 and s in (1, 2):
        return _pack_conv3x3(w, b, relu, s)
    kind, packer = _POINTWISE.get((transposed, k, s), (None, None))
    if kind is None:
        raise NotImplementedError('%s k=%d s=%d has no HIP kernel in this build' % ('ConvTranspose2d' if transposed else 'Conv2d', k, s))
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    pc = PackedConv(kind, cin, cout, relu, packer(w, b))
    _pack_mp_pointwise(pc)
    return pc


def pack_conv_raw(w, b, relu, stride=1):
    """3x3 conv from an explicit (already folded) weight/bias pair, e.g. the fused CenterHead branches."""
    return _pack_conv3x3(w, b, relu, stride)
