"""Hand-rolled forward/backward of the dense layers for the training path (no torch.autograd inside): every layer saves what its
backward needs, `backward(dout)` writes parameter gradients straight into `param.grad` and returns the input gradient.

A conv layer of the trainable branch is  y = conv(x) [+ bias];  a = relu?(bn_train?(y)).
  forward   conv    -> with the RAW weights (no BN folding, relu = 0).  3x3, fp32: the kernel conv_dispatch.choose_train_conv3x3 names --
                       pcp_conv3x3_bf16x3 (opt-in), the fused F(4x4) kernels pcp_conv3x3_winograd4f / _winograd4h (stride 1, chosen at pack
                       time by fused_f4_choice), pcp_conv3x3_winograd (fused F(2x2), stride 1) or pcp_conv3x3;  3x3 in the bf16 loop
                       (PCP_CONV_ALGO=bf16, mp_mode()): pcp_mp_conv3x3;  1x1 / k2 s2 kinds: pcp_pointwise, or pcp_mp_pointwise where a
                       bf16 map arrives in the bf16 loop
            bn      -> pcp_bn_train_stats (batch statistics, running stats updated) + pcp_scale_shift_act
  backward  bn+relu -> pcp_bn_act_backward (in place on the incoming gradient)
            bias    -> pcp_colsum
            wgrad   -> pcp_conv3x3_wgrad / pcp_mp_conv3x3_wgrad / pcp_pointwise_wgrad (pixel-contraction MFMA GEMMs)
            dgrad   -> the FORWARD kernels again with flipped / transposed weights (stride-2 3x3: on the zero-dilated gradient, pcp_dilate2x)
  weights   TrainForms: packed once per optimizer step -- per layer at its first step (pcp_pack_conv3x3, pcp_pack_conv3x3_winograd4,
            pcp_mp_pack_conv3x3), afterwards every 3x3 layer by ONE launch (pcp_pack_conv3x3_group / pcp_mp_pack_conv3x3_group)

Reference modules these stand for: nn.Conv2d / nn.ConvTranspose2d + nn.BatchNorm2d + nn.ReLU stacks of
pcdet/models/backbones_2d/base_bev_backbone.py:30-69, dense_heads/center_head.py:24-29,75-82, bev_layers/v2x_fusion_disco.py:11-17,51-63.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import lib, ops, pack
from . import train_ops as tops
from .conv_dispatch import Forms, choose_fused_f4, choose_train_conv3x3, conv_algo, fused_f4_shape


def fused_f4_choice(B, H, W, cin, cout):
    """which fused Winograd F(4x4,3x3) kernel a stride-1 3x3 conv cin -> cout on a (B, H, W) map goes to in the training step: None | '4f' |
    '4h'.  The rule of the inference dispatch (conv_dispatch.choose_fused_f4): k_wino4h up to 128 input channels or where k_wino4f's
    16 x 32-pixel items leave CUs idle, k_wino4f for the wider layers, neither below one item per CU slot.  PCP_CONV_ALGO = winograd4f |
    winograd4h forces a kernel (tests), direct | winograd | bf16* switch both off.  The keyword arguments are where this rule differs from
    inference (each explained at choose_fused_f4)."""
    algo = conv_algo()
    if not fused_f4_shape(cin, cout, 1, algo):
        return None
    name = choose_fused_f4(algo, cin, pack.round_up(cout, 64), False, B, H, W, kernel_limits=False, knows_4c=False, wino4h_overrides=False,
                           cap_needs_w4=False, half_before_cap=True)
    return {'winograd4f': '4f', 'winograd4h': '4h'}.get(name)


def mp_mode():
    """PCP_CONV_ALGO=bf16: the mixed-precision training loop (include/pcp_hip_mp.h) -- the 3x3 layers store their activations and
    gradients as bf16 and run forward / data-gradient / weight-gradient on the bf16 matrix cores; master weights, BatchNorm, losses
    and the optimizer stay fp32"""
    return conv_algo() == 'bf16'


def as_f32(t, off=0, c=None):
    """contiguous float32 copy of a channel window (the fp32-only kernels' view of a bf16 activation); fp32 full-width input: itself"""
    c = t.shape[-1] - off if c is None else c
    if t.dtype == torch.float32 and off == 0 and c == t.shape[-1]:
        return t
    return t[..., off:off + c].float().contiguous()


def as_bf16(t, off=0, c=None):
    c = t.shape[-1] - off if c is None else c
    if t.dtype == torch.bfloat16 and off == 0 and c == t.shape[-1]:
        return t
    return t[..., off:off + c].to(torch.bfloat16).contiguous()


PACK_GROUP = tops.PackGroup()
MP_PACK_GROUP = tops.MpPackGroup()
PACK_GROUPING = os.environ.get('PCP_PACK_GROUP', '1') != '0'


class StepClock:
    """Packed weights are rebuilt when the optimizer has stepped (weights change through raw pointers, torch cannot tell)."""
    step = 0

    @classmethod
    def tick(cls):
        cls.step += 1
        flush_batches_tracked()


# nn.BatchNorm's num_batches_tracked += 1 is one tiny launch per BatchNorm per forward (47 per DiscoNet iteration): the increments are
# collected and applied by ONE multi-tensor add per optimizer step, and before any state_dict(): PackedModule and Detector3DTemplate register
# flush_batches_tracked() as a state_dict pre-hook, so a checkpoint taken between a forward and optimizer.step() carries current counters.
_PENDING_NBT = {}


def bump_batches_tracked(bn):
    t = bn.num_batches_tracked
    if t is None:
        return
    e = _PENDING_NBT.get(id(t))
    if e is None:
        _PENDING_NBT[id(t)] = [t, 1]
    else:
        e[1] += 1
    if len(_PENDING_NBT) > 4096:
        flush_batches_tracked()


def drop_pending_batches_tracked(module):
    """forget the collected increments of `module`'s BatchNorm counters (they were just replaced by load_state_dict: adding increments
    from before the load would corrupt the loaded values)"""
    if not _PENDING_NBT:
        return
    for name, buf in module.named_buffers():
        if name.endswith('num_batches_tracked'):
            _PENDING_NBT.pop(id(buf), None)


def flush_batches_tracked():
    if not _PENDING_NBT:
        return
    by_count = {}
    for t, n in _PENDING_NBT.values():
        by_count.setdefault((n, t.device), []).append(t)
    _PENDING_NBT.clear()
    for (n, _dev), ts in by_count.items():
        torch._foreach_add_(ts, n)


def ensure_grad(p):
    if p.grad is None or p.grad.shape != p.shape or p.grad.device != p.device or not p.grad.is_contiguous():
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


class Act:
    """a channel window of an NHWC (or row-major) buffer"""
    __slots__ = ('t', 'off', 'c')

    def __init__(self, t, off=0, c=None):
        self.t, self.off, self.c = t, off, (t.shape[-1] - off if c is None else c)

    @property
    def rows(self):
        return self.t.numel() // self.t.shape[-1]


def _bf16_window(a):
    """the Act as the bf16 kernels read it: bf16 storage, window and row pitch multiples of 8 channels (16 bytes) -- itself where it already
    is one, else ONE cast into a contiguous copy of the window"""
    if a.t.dtype != torch.bfloat16 or a.off % 8 or a.t.shape[-1] % 8:
        return Act(as_bf16(a.t, a.off, a.c), 0, a.c)
    return a


_ZERO_BIAS = {}


def _zero_bias(device):
    z = _ZERO_BIAS.get(device)
    if z is None:
        z = _ZERO_BIAS[device] = torch.zeros(2048, dtype=torch.float32, device=device)
    return z


Form = namedtuple('Form', 'w b cout_pad')          # one packed weight form: (weights, bias, cout_pad)


class ConvForms:
    """the packed forms of ONE direction of a conv (forward | data gradient), None where it has none.  3x3: direct (always), wino (fused
    F(2x2)), b3 (split bf16), f4 (fused F(4x4), packed for the kernel f4_kernel names) -- or mp alone in the bf16 loop.  Pointwise kinds:
    direct, and mp (its bf16 copy) in the bf16 loop."""
    __slots__ = ('direct', 'wino', 'b3', 'f4', 'f4_kernel', 'mp')

    def __init__(self, direct=None, wino=None, b3=None, f4=None, f4_kernel=None, mp=None):
        self.direct, self.wino, self.b3, self.f4, self.f4_kernel, self.mp = direct, wino, b3, f4, f4_kernel, mp


# kernel name of conv_dispatch.choose_train_conv3x3 -> (slot of ConvForms, function of pcp_amd.ops, looked up at every call: tests replace them)
_LAUNCH3X3 = {'direct': ('direct', 'conv3x3'), 'winograd': ('wino', 'conv3x3_winograd'), 'winograd4f': ('f4', 'conv3x3_winograd4f'),
              'winograd4h': ('f4', 'conv3x3_winograd4h'), 'bf16x3': ('b3', 'conv3x3_bf16x3')}


def launch_conv3x3(forms, x, cin, cout, stride, out, in_off, out_off):
    """the fp32 3x3 conv cin -> cout of a training step (a layer's forward, or a stride-1 data-gradient conv) from x[..., in_off:] into
    out[..., out_off:], on the kernel conv_dispatch.choose_train_conv3x3 names, with the ConvForms `forms`"""
    B, H, W, ld_in = x.shape
    algo = conv_algo()
    pads = Forms(wino=forms.wino and forms.wino.cout_pad, b3=forms.b3 and forms.b3.cout_pad)
    name = choose_train_conv3x3(algo, stride, pads, forms.f4_kernel, B, H, W, ld_in, in_off, out.shape[-1], out_off)
    slot, fn = _LAUNCH3X3[name]
    w, b, cp = getattr(forms, slot)
    extra = {}
    if name in ('direct', 'bf16x3'):                       # the two kernels that also take stride 2
        extra['stride'] = stride
    if name == 'bf16x3':
        extra['plain'] = algo == 'bf16'
    return getattr(ops, fn)(x, w, b, cin, cout, cp, relu=False, out=out, in_ch_off=in_off, out_ch_off=out_off, **extra)


class TrainForms:
    """The packed weight forms of one conv module in the training step.  Cached ON THE MODULE (several layers may share one: the weightor
    runs once per agent) and rebuilt once per optimizer step, by one of three packers.  The 3x3 forms live in persistent buffers: the first
    pack of a layer writes them with its own launches and registers them with PACK_GROUP / MP_PACK_GROUP, and from the next step on ONE launch
    per step rewrites the buffers of every registered layer through their raw pointers."""

    def __init__(self, kind, cin, cout, stride):
        self.kind, self.cin, self.cout, self.stride = kind, cin, cout, stride
        self.step = -1                  # StepClock.step the forms were packed at
        self.f4_key = None              # ((B, H, W), PCP_CONV_ALGO) self.f4 was chosen for
        self.f4 = (None, None)          # fused_f4_choice of (the forward conv, the data-gradient conv)
        self.fw = self.bw = None        # ConvForms
        self.buf = {}                   # (transpose, slot) -> persistent buffer of a 3x3 form; slots direct, wino, b3, 4f, 4h, mp

    def get(self, conv, bhw):
        """(forward ConvForms, data-gradient ConvForms) of `conv`, current for this optimizer step.  bhw: (B, H, W) of the layer input -- decides
        whether the fused F(4x4) forms are packed (forward: the conv on that map; data gradient: the stride-1 conv on the same map, for stride
        2 on the zero-dilated gradient)"""
        if self._stale(conv, bhw):
            if self.kind != '3x3':
                self._pack_pointwise(conv)
            elif mp_mode() and self.cin % 16 == 0 and self.cout % 16 == 0:
                self._pack_bf16_3x3(conv)
            else:
                self._pack_fp32_3x3(conv)
            self.step = StepClock.step
        return self.fw, self.bw

    def _stale(self, conv, bhw):
        """has the optimizer stepped, or has the fused-F(4x4) choice changed, since the forms were packed"""
        if self.kind == '3x3' and self.f4_key != (bhw, conv_algo()):
            self.f4_key = (bhw, conv_algo())
            f4 = (fused_f4_choice(*bhw, self.cin, self.cout) if self.stride == 1 else None, fused_f4_choice(*bhw, self.cout, self.cin))
            if f4 != self.f4:
                # another fused form is needed (another batch / map shape, e.g. the last partial batch): pack per layer once, so that the new
                # form is packed AND registered -- the group launch only rewrites the forms it was given
                self.f4, self.step = f4, -1
                PACK_GROUP.drop((id(conv), False))
                PACK_GROUP.drop((id(conv), True))
        return self.step != StepClock.step

    @staticmethod
    def _in_group(group, conv, w):
        return group.has((id(conv), False), w.data_ptr()) and group.has((id(conv), True), w.data_ptr())

    def _pack_bf16_3x3(self, conv):
        """bf16 loop: the bf16 forms (forward + data gradient) from the fp32 master weights"""
        w = conv.weight.detach()
        wc = w if w.is_contiguous() else w.contiguous()
        fo, bo = pack.round_up(self.cout, 64), pack.round_up(self.cin, 64)
        fwp, bwp = self.buf.get((False, 'mp')), self.buf.get((True, 'mp'))
        if fwp is not None and self._in_group(MP_PACK_GROUP, conv, w):
            MP_PACK_GROUP.run_once(StepClock.step, w.device)
        else:
            fwp, fo = tops.mp_pack_conv3x3(wc, False, out=fwp)
            bwp, bo = tops.mp_pack_conv3x3(wc, True, out=bwp)
            self.buf[False, 'mp'], self.buf[True, 'mp'] = fwp, bwp
            if PACK_GROUPING and wc.data_ptr() == w.data_ptr():       # the parameter's own storage: later steps go through the group launch
                MP_PACK_GROUP.add((id(conv), False), conv, wc, False, fwp, fo)
                MP_PACK_GROUP.add((id(conv), True), conv, wc, True, bwp, bo)
        zeros = _zero_bias(w.device)
        b = conv.bias.detach() if conv.bias is not None else None
        fb = zeros if b is None else (b if fo == self.cout else pack.pad_bias(b, fo))
        self.fw, self.bw = ConvForms(mp=Form(fwp, fb, fo)), ConvForms(mp=Form(bwp, zeros, bo))

    def _alloc_fp32_3x3(self, dev):
        """the persistent buffers of the fp32 forms a layer has whatever its map: direct; wino and b3 where the kernels take the shape"""
        rp = lambda o: pack.round_up(o, 64 if o > 32 else 32)
        for tr, i, o in ((False, self.cin, self.cout), (True, self.cout, self.cin)):
            self.buf[tr, 'direct'] = torch.empty((i // 16, 9, rp(o), 16), dtype=torch.float32, device=dev)
            if (tr or self.stride == 1) and i % pack.WINO_CK == 0 and o >= 48:
                self.buf[tr, 'wino'] = torch.empty((i // 8, 16, pack.round_up(o, 64), 8), dtype=torch.float32, device=dev)
            if conv_algo() in ('bf16x3', 'bf16') and i % 16 == 0 and o >= 48:      # opt-in split / plain bf16 arithmetic (conv_bf16x3.hip)
                self.buf[tr, 'b3'] = torch.empty((i // 16) * pack.round_up(o, 64) * 9 * 16 * 2, dtype=torch.int16, device=dev)

    def _pack_fp32_3x3(self, conv):
        """the fp32 forms: pcp_pack_conv3x3 writes direct / wino / b3 (one launch per direction), pcp_pack_conv3x3_winograd4 the fused form"""
        w = conv.weight.detach()
        dev = w.device
        if self.fw is not None and self.fw.direct is not None and self._in_group(PACK_GROUP, conv, w):
            PACK_GROUP.run_once(StepClock.step, dev)         # the forms stay: their buffers were rewritten
            return
        buf = self.buf
        if (False, 'direct') not in buf:
            self._alloc_fp32_3x3(dev)
        zeros = _zero_bias(dev)
        b = conv.bias.detach() if conv.bias is not None else None
        wc = w.contiguous()
        dirs = ((False, self.cin, self.cout, self.f4[0]), (True, self.cout, self.cin, self.f4[1]))
        pad = lambda t: t.shape[2] if t is not None else 0
        for tr, i, o, _f4 in dirs:
            d, wi = buf[tr, 'direct'], buf.get((tr, 'wino'))
            tops.pack_conv3x3(wc, tr, d, pad(d), wi, pad(wi), buf.get((tr, 'b3')), pack.round_up(o, 64))
        for tr, i, o, f4 in dirs:
            if f4 is not None:
                if (tr, f4) not in buf:
                    buf[tr, f4] = torch.empty((i // 8) * 36 * pack.round_up(o, 64) * 8, dtype=torch.float32, device=dev)
                tops.pack_conv3x3_winograd4(wc, tr, buf.get((tr, f4)) if f4 == '4f' else None, buf.get((tr, f4)) if f4 == '4h' else None,
                                            pack.round_up(o, 64))
        forms = []
        for tr, i, o, f4 in dirs:
            def bias(n_pad):                                 # forward: the conv bias, padded (a per-step copy); data gradient: none
                return zeros if (tr or b is None) else (b if n_pad == o else pack.pad_bias(b, n_pad))
            f, o64 = ConvForms(), pack.round_up(o, 64)
            if f4 is not None:
                f.f4, f.f4_kernel = Form(buf[tr, f4], bias(o64), o64), 'winograd' + f4
            d, wi, b3 = buf[tr, 'direct'], buf.get((tr, 'wino')), buf.get((tr, 'b3'))
            f.direct = Form(d, bias(pad(d)), pad(d))
            if wi is not None:
                f.wino = Form(wi, bias(pad(wi)), pad(wi))
            if b3 is not None:
                f.b3 = Form(b3, bias(o64), o64)
            forms.append(f)
        self.fw, self.bw = forms
        if PACK_GROUPING and b is None and self.fw.b3 is None and self.bw.b3 is None and wc.data_ptr() == w.data_ptr():
            # the buffers are persistent, no bias is copied and the weight tensor is the parameter's own storage: later steps repack through
            # the group launch
            for (tr, i, o, f4), f in zip(dirs, forms):
                wi = buf.get((tr, 'wino'))
                PACK_GROUP.add((id(conv), tr), conv, wc, tr, buf[tr, 'direct'], f.direct.cout_pad, wi, pad(wi),
                               buf[tr, f4] if f4 == '4f' else None, buf[tr, f4] if f4 == '4h' else None, f.f4.cout_pad if f.f4 else 0)

    def _pack_pointwise(self, conv):
        """the four pointwise kinds: packed by torch (pack.py) every step; in the bf16 loop also as bf16 for pcp_mp_pointwise (used when the
        layer's input arrives as bf16)"""
        w = conv.weight.detach()
        dev = w.device
        cin, cout, k = self.cin, self.cout, self.kind
        zeros = _zero_bias(dev)
        fb = conv.bias.detach() if conv.bias is not None else zeros[:cout]
        zb = zeros[:cin]
        if k == 'plain':
            m = w.reshape(cout, cin)
            fw, bw = pack.pack_plain(m, fb), pack.pack_plain(m.t().contiguous(), zb)
        elif k == 'plainT':
            m = w.reshape(cin, cout)
            fw, bw = pack.pack_plain(m.t().contiguous(), fb), pack.pack_plain(m.contiguous(), zb)
        elif k == 's2d':
            fw, bw = pack.pack_conv2x2_s2(w, fb), pack.pack_convT2x2_s2(w, zb)     # (cout, cin, 2, 2) read as a ConvTranspose2d weight
        else:  # d2s
            fw, bw = pack.pack_convT2x2_s2(w, fb), pack.pack_conv2x2_s2(w, zb)     # (cin, cout, 2, 2) read as a Conv2d weight
        self.fw, self.bw = ConvForms(direct=Form(*fw)), ConvForms(direct=Form(*bw))
        if mp_mode() and dev.type == 'cuda':
            for f, i, o in ((self.fw, cin, cout), (self.bw, cout, cin)):
                if tops.mp_pointwise_ok(None, i, o, f.direct.cout_pad, 8, 8):
                    f.mp = Form(f.direct.w.to(torch.bfloat16), f.direct.b, f.direct.cout_pad)


_PW_FORWARD = {'plain': lib.PW_PLAIN, 'plainT': lib.PW_PLAIN, 's2d': lib.PW_SPACE2DEPTH, 'd2s': lib.PW_DEPTH2SPACE}
_PW_BACKWARD = {'plain': lib.PW_PLAIN, 'plainT': lib.PW_PLAIN, 's2d': lib.PW_DEPTH2SPACE, 'd2s': lib.PW_SPACE2DEPTH}


class ConvBNAct:
    """kind: '3x3' (stride 1 | 2, padding 1), 'plain' (Conv2d 1x1), 'plainT' (ConvTranspose2d 1x1), 's2d' (Conv2d k2 s2),
    'd2s' (ConvTranspose2d k2 s2)."""

    def __init__(self, conv, bn=None, relu=True, name=''):
        self.conv, self.bn, self.relu, self.name = conv, bn, relu, name
        k, s = conv.kernel_size[0], conv.stride[0]
        if isinstance(conv, nn.ConvTranspose2d):
            self.cin, self.cout = conv.weight.shape[0], conv.weight.shape[1]
            self.kind = {(1, 1): 'plainT', (2, 2): 'd2s'}.get((k, s))
        else:
            self.cout, self.cin = conv.weight.shape[0], conv.weight.shape[1]
            self.kind = {(3, 1): '3x3', (3, 2): '3x3', (1, 1): 'plain', (2, 2): 's2d'}.get((k, s))
        if self.kind is None:
            raise NotImplementedError('%s: conv k=%d s=%d has no training kernel' % (name, k, s))
        self.stride = s if self.kind == '3x3' else 1
        self._fw = self._bw = None      # ConvForms of the current step
        self._mpw = False               # a pointwise layer whose last forward ran in the bf16 loop
        self.saved = None
        self.vec = None

    def _current_forms(self, x):
        """the weight forms of this step, for a layer input x (a tensor): self._fw, self._bw"""
        forms = getattr(self.conv, '_pcp_train_forms', None)
        if forms is None:
            forms = self.conv._pcp_train_forms = TrainForms(self.kind, self.cin, self.cout, self.stride)
        self._fw, self._bw = forms.get(self.conv, tuple(x.shape[:3]))

    def mp_pointwise_capable(self):
        """a pointwise layer whose forward AND data-gradient shapes pcp_mp_pointwise takes (it then reads and writes bf16 maps)"""
        rp = lambda o: pack.round_up(o, 64 if o > 32 else 32)
        return (self.kind != '3x3' and mp_mode() and tops.mp_pointwise_ok(None, self.cin, self.cout, rp(self.cout), 8, 8)
                and tops.mp_pointwise_ok(None, self.cout, self.cin, rp(self.cin), 8, 8))

    def out_shape(self, x):
        B, H, W = x.t.shape[0], x.t.shape[1], x.t.shape[2]
        if self.kind == '3x3':
            return (B, H // self.stride, W // self.stride)
        if self.kind == 's2d':
            return (B, H // 2, W // 2)
        if self.kind == 'd2s':
            return (B, 2 * H, 2 * W)
        return (B, H, W)

    def forward(self, x, out=None, out_dtype=None):
        """x: Act.  out: Act to write the activation into (a channel window of a wider buffer) or None.  Returns Act.
        Mixed-precision mode (mp_mode()): a 3x3 layer takes fp32 or bf16 input, keeps its conv output as bf16 and writes its activation
        as bf16 unless `out` / `out_dtype` say float32 (a consumer that is an fp32-only kernel); the other kinds compute in fp32."""
        self._current_forms(x.t)
        fw = self._fw
        dev = x.t.device
        shp = self.out_shape(x)
        need_post = self.bn is not None or self.relu
        k = self.kind
        mp = k == '3x3' and fw.mp is not None
        # a pointwise layer joins the bf16 loop when its input ARRIVES as bf16 (the up / down-sampling layers behind the bf16 3x3 blocks);
        # fp32 inputs (the fusion module's concatenated maps) keep the fp32 kernels
        mpw = (k != '3x3' and fw.mp is not None and self._bw.mp is not None and x.t.dtype == torch.bfloat16 and x.off % 8 == 0
               and x.t.shape[-1] % 8 == 0 and (out is None or (out.off % 8 == 0 and out.t.shape[-1] % 8 == 0)))
        if mp or mpw:
            if mp:
                x = _bf16_window(x)                                      # the fast kernel and the weight gradient both read the bf16 copy
            act_dtype = out.t.dtype if out is not None else (out_dtype or torch.bfloat16)
            y_dtype = torch.bfloat16 if need_post else act_dtype
        else:
            if x.t.dtype != torch.float32:
                x = Act(as_f32(x.t, x.off, x.c), 0, x.c)
            act_dtype = y_dtype = torch.float32
            if out is not None and out.t.dtype != torch.float32:
                raise NotImplementedError('%s: fp32 layer kind %s cannot write a bf16 buffer' % (self.name, k))
        y_t = torch.empty(shp + (self.cout,), dtype=y_dtype, device=dev) if (need_post or out is None) else None
        y = Act(y_t, 0, self.cout) if y_t is not None else out
        if mp:
            wp, bp, cp = fw.mp
            tops.mp_conv3x3(x.t, wp, bp, self.cin, self.cout, cp, stride=self.stride, relu=False, out=y.t, in_ch_off=x.off, out_ch_off=y.off)
        elif k == '3x3':
            launch_conv3x3(fw, x.t, self.cin, self.cout, self.stride, y.t, x.off, y.off)
        else:
            (w, b, cp), run = (fw.mp, tops.mp_pointwise) if mpw else (fw.direct, ops.pointwise)
            run(x.t, w, b, _PW_FORWARD[k], self.cin, self.cout, cp, relu=False, out=y.t, in_ch_off=x.off, out_ch_off=y.off)
        self._mpw = mpw
        if not need_post:
            self.saved = (x, y)
            return y
        if out is None:
            out = Act(torch.empty(shp + (self.cout,), dtype=act_dtype, device=dev), 0, self.cout)
        if self.bn is not None:
            bn = self.bn
            self.vec = tops.bn_train_stats(y.t, self.cout, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum,
                                           bn.running_mean, bn.running_var, vec=self.vec, ch_off=y.off)
            bump_batches_tracked(bn)
        else:
            if self.vec is None:
                self.vec = tops.BNVectors(self.cout, dev)
                self.vec.scale.fill_(1.0)
                self.vec.shift.zero_()
        tops.scale_shift_act(y.t, self.cout, self.vec, self.relu, out.t, in_ch_off=y.off, out_ch_off=out.off)
        self.saved = (x, y)
        return out

    def _weight_grad(self, x, dy, mp, accumulate):
        """dL/d conv.weight from the saved input x and the conv-output gradient dy (both Act), into conv.weight.grad"""
        k, cin, cout = self.kind, self.cin, self.cout
        gw = ensure_grad(self.conv.weight)
        if k == '3x3':
            wgrad = tops.mp_conv3x3_wgrad if mp else tops.conv3x3_wgrad
            wgrad(x.t, dy.t, cin, cout, self.stride, gw, accumulate=accumulate, x_ch_off=x.off, dy_ch_off=dy.off)
        elif k == 'plain':
            tops.pointwise_wgrad(tops.rowmap(dy.t, cout, dy.off), tops.rowmap(x.t, cin, x.off), x.rows, gw.view(cout, cin), accumulate=accumulate)
        elif k == 'plainT':
            tops.pointwise_wgrad(tops.rowmap(x.t, cin, x.off), tops.rowmap(dy.t, cout, dy.off), x.rows, gw.view(cin, cout), accumulate=accumulate)
        else:
            # k2 s2: one GEMM per tap, between the coarse map and the tap's lattice of the fine one.  s2d: fine x, coarse dy, (cout, cin) taps;
            # d2s: coarse x, fine dy, (cin, cout) taps
            (n, fine), (m, coarse) = ((cin, x), (cout, dy)) if k == 's2d' else ((cout, dy), (cin, x))
            H, W = coarse.t.shape[1], coarse.t.shape[2]
            tmp = torch.empty((4, m, n), dtype=torch.float32, device=dy.t.device)
            for tap in range(4):
                tops.pointwise_wgrad(tops.rowmap(coarse.t, m, coarse.off), tops.rowmap(fine.t, n, fine.off, lattice=(H, W, tap // 2, tap % 2)),
                                     coarse.rows, tmp[tap])
            g = tmp.permute(1, 2, 0).reshape(m, n, 2, 2)
            gw.add_(g) if accumulate else gw.copy_(g)

    def backward(self, dout, need_dx=True, accumulate=False, dx_out=None, dx_dtype=None):
        """dout: Act (gradient of the layer output; overwritten in place by the gradient of the conv output when the storage types allow).
        Returns Act dx (or None).  accumulate: add to param.grad instead of overwriting (a module applied several times).
        Mixed-precision 3x3 layers take fp32 or bf16 gradients, keep the conv-output gradient as bf16 (the operand of both gradient
        GEMMs) and return dx as bf16 unless dx_out / dx_dtype say float32."""
        x, y = self.saved
        dev = dout.t.device
        k = self.kind
        mp = self._fw.mp is not None if k == '3x3' else self._mpw       # bf16 operands for both gradient GEMMs
        if not mp and dout.t.dtype != torch.float32:
            dout = Act(as_f32(dout.t, dout.off, dout.c), 0, dout.c)
        if self.bn is not None:
            g_w, g_b = ensure_grad(self.bn.weight), ensure_grad(self.bn.bias)
            # in place on dout, whatever its storage type (callers rely on it: the CenterHead runs ONE data-gradient conv over the five
            # branch gradients it handed to five layers)
            tops.bn_act_backward(dout.t, y.t, self.cout, self.vec, self.relu, g_w, g_b, accumulate=accumulate, dout_ch_off=dout.off,
                                 x_ch_off=y.off)
        elif self.relu:
            raise NotImplementedError('%s: ReLU without BatchNorm is handled by the fused fusion kernels' % self.name)
        dy = _bf16_window(dout) if mp else dout
        if self.conv.bias is not None:
            tops.colsum(dy.t, self.cout, ensure_grad(self.conv.bias), accumulate=accumulate, ch_off=dy.off)
        self._weight_grad(x, dy, mp, accumulate)
        if not need_dx:
            return None
        self._current_forms(x.t)
        bw = self._bw
        if dx_out is None:
            dt = (dx_dtype or torch.bfloat16) if mp else torch.float32
            dx_out = Act(torch.empty(tuple(x.t.shape[:-1]) + (self.cin,), dtype=dt, device=dev), 0, self.cin)
        if k == '3x3':
            # the forward kernels again with flipped / transposed weights; stride 2: a stride-1 conv on the zero-dilated gradient
            src = dy if self.stride == 1 else Act(tops.dilate2x(dy.t, self.cout, ch_off=dy.off), 0, self.cout)
            if mp:
                wp, bp, cp = bw.mp
                tops.mp_conv3x3(src.t, wp, bp, self.cout, self.cin, cp, stride=1, relu=False, out=dx_out.t, in_ch_off=src.off,
                                out_ch_off=dx_out.off)
            else:
                launch_conv3x3(bw, src.t, self.cout, self.cin, 1, dx_out.t, src.off, dx_out.off)
        else:
            (w, b, cp), run = (bw.mp, tops.mp_pointwise) if mp else (bw.direct, ops.pointwise)
            run(dy.t, w, b, _PW_BACKWARD[k], self.cout, self.cin, cp, relu=False, out=dx_out.t, in_ch_off=dy.off, out_ch_off=dx_out.off)
        return dx_out


class LinearBNAct:
    """nn.Linear (no bias) + BatchNorm1d (batch statistics) + ReLU on rows (N, cin) -- the blocks of hunter_toolbox.py:130-158 (nn_make_mlp).
    cin is padded to a multiple of 16 with zero weight columns (the 3-d and 774-d inputs of the object head)."""

    def __init__(self, linear, bn, relu=True, name=''):
        self.lin, self.bn, self.relu, self.name = linear, bn, relu, name
        self.cout, self.cin = linear.weight.shape
        self.cin_pad = pack.round_up(self.cin, 16)
        assert linear.bias is None and bn is not None
        self._step = -1
        self.vec = None
        self.saved = None

    def _forms(self):
        if self._step == StepClock.step:
            return self._f
        w = self.lin.weight.detach().float()
        dev = w.device
        wp = w.new_zeros((self.cout, self.cin_pad))
        wp[:, :self.cin] = w
        self._f = dict(fw=pack.pack_plain(wp, w.new_zeros(self.cout)), bw=pack.pack_plain(wp.t().contiguous(), w.new_zeros(self.cin_pad)))
        self._step = StepClock.step
        return self._f

    def forward(self, x):
        """x: (rows, ld >= cin_pad) contiguous, columns [cin, cin_pad) zero.  Returns (rows, cout)."""
        f = self._forms()
        rows = x.shape[0]
        w, b, cp = f['fw']
        y = torch.empty((rows, self.cout), dtype=torch.float32, device=x.device)
        ops.pointwise(x, w, b, lib.PW_PLAIN, self.cin_pad, self.cout, cp, relu=False, out=y)
        bn = self.bn
        self.vec = tops.bn_train_stats(y, self.cout, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                                       vec=self.vec)
        bump_batches_tracked(bn)
        out = torch.empty_like(y)
        tops.scale_shift_act(y, self.cout, self.vec, self.relu, out)
        self.saved = (x, y)
        return out

    def backward(self, dout, need_dx=True):
        """dout: (rows, cout), overwritten.  Returns (rows, cin_pad) or None."""
        x, y = self.saved
        tops.bn_act_backward(dout, y, self.cout, self.vec, self.relu, ensure_grad(self.bn.weight), ensure_grad(self.bn.bias))
        rows = x.shape[0]
        dw = torch.empty((self.cout, self.cin_pad), dtype=torch.float32, device=x.device)
        tops.pointwise_wgrad(tops.rowmap(dout, self.cout), tops.rowmap(x, self.cin_pad), rows, dw)
        ensure_grad(self.lin.weight).copy_(dw[:, :self.cin])
        if not need_dx:
            return None
        w, b, cp = self._forms()['bw']
        dx = torch.empty((rows, self.cin_pad), dtype=torch.float32, device=x.device)
        ops.pointwise(dout, w, b, lib.PW_PLAIN, self.cout, self.cin_pad, cp, relu=False, out=dx)
        return dx


class MultiLinear:
    """several nn.Linear (with bias) reading the same rows, as ONE pointwise GEMM over the concatenated outputs (the three point heads
    seg / reg_flow3d / instance_embedding of hunter_jr.py:93-96, the local_tf_decoder of :40).  The output / gradient buffers are 16 columns
    wide per 16 outputs so that the gradient is a legal contraction operand of the data-gradient GEMM."""

    def __init__(self, linears, name=''):
        self.lins, self.name = list(linears), name
        self.outs = [l.weight.shape[0] for l in self.lins]
        self.offs = [0]
        for o in self.outs:
            self.offs.append(self.offs[-1] + o)
        self.cin = self.lins[0].weight.shape[1]
        self.cout = self.offs[-1]
        self.ld = pack.round_up(self.cout, 16)
        self._step = -1
        self.saved = None

    def _forms(self):
        if self._step == StepClock.step:
            return self._f
        w = torch.cat([l.weight.detach().float() for l in self.lins], 0)
        b = torch.cat([l.bias.detach().float() for l in self.lins], 0)
        wt = w.new_zeros((self.cin, self.ld))
        wt[:, :self.cout] = w.t()
        self._f = dict(fw=pack.pack_plain(w, b), bw=pack.pack_plain(wt, w.new_zeros(self.cin)))
        self._step = StepClock.step
        return self._f

    def forward(self, x):
        """x: (rows, cin) contiguous.  Returns (rows, ld); columns past cout are zero."""
        w, b, cp = self._forms()['fw']
        out = torch.zeros((x.shape[0], self.ld), dtype=torch.float32, device=x.device)
        ops.pointwise(x, w, b, lib.PW_PLAIN, self.cin, self.cout, cp, relu=False, out=out)
        self.saved = x
        return out

    def backward(self, dout):
        """dout: (rows, ld) with zero padding columns.  Returns (rows, cin)."""
        x = self.saved
        rows = x.shape[0]
        dw = torch.empty((self.ld, self.cin), dtype=torch.float32, device=x.device)
        tops.pointwise_wgrad(tops.rowmap(dout, self.ld), tops.rowmap(x, self.cin), rows, dw)
        db = torch.empty((self.ld,), dtype=torch.float32, device=x.device)
        tops.colsum(dout, self.ld, db)
        for i, l in enumerate(self.lins):
            ensure_grad(l.weight).copy_(dw[self.offs[i]:self.offs[i + 1]])
            ensure_grad(l.bias).copy_(db[self.offs[i]:self.offs[i + 1]])
        w, b, cp = self._forms()['bw']
        dx = torch.empty((rows, self.cin), dtype=torch.float32, device=x.device)
        ops.pointwise(dout, w, b, lib.PW_PLAIN, self.ld, self.cin, cp, relu=False, out=dx)
        return dx
