"""Recorder of the training conv layer's launches: tests/golden/train_conv_table.json.

Which kernel every launch of `train_layers.ConvBNAct` (and of the CenterHead branches, `train_path._HeadBranches`) runs, which packed weight
form it reads, when the forms are repacked and what the per-step group launch is told to write are host-side decisions, so they are recorded
on the CPU through the public surface only: `ConvBNAct(conv, bn, relu)`, `.forward(Act)`, `.backward(Act, ...)`, `StepClock.tick()`,
`_HeadBranches.forward / .backward`.  The `ops.*` and `train_ops.*` functions the layers call are replaced by stubs that note their name, their
scalar arguments and the shape and storage type of their tensors; a packed weight is noted as the role of the form it belongs to (the role
is learned when a packing stub is handed the destination buffer: 'c.fw.direct', 'c.bw.f4h', ...), a bias as zero or non-zero.  The four
library symbols of the group repack and `train_ops._stream` are replaced by fakes, so `PackGroup.add` / `.run` and `MpPackGroup.add` / `.run`
execute: the fake launch reads the uploaded job table back and notes every job with the roles of the buffers its raw pointers name.
tests/test_host_cpu.py runs `record()` again and demands equality with the committed file on every row.

3x3 rows run on `meta` activations (the rule depends on the map size, nothing is computed), pointwise and head rows on small CPU tensors, and
the pointwise rows of the bf16 loop on fake `cuda` tensors (the bf16 pointwise forms are only made for weights on the GPU) in a child process
that is shown no GPU.

    python tests/golden/make_train_conv_table.py          # rewrites the JSON; the file names the commit it was recorded at
"""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, 'practical-collab-perception_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
TABLE = os.path.join(HERE, 'train_conv_table.json')

ALGOS = [None, 'auto', 'direct', 'winograd', 'winograd4', 'winograd4f', 'winograd4h', 'winograd4c', 'bf16x3', 'bf16', 'no-such-algo']
# (cin, cout): both sides of cout >= 48 (F(2x2) / bf16x3 / fused forms), of 128 input channels (k_wino4h | k_wino4f), of the bf16 loop's
# 16-channel condition (56 and 40 outputs), a cin that is a multiple of 8 on both sides of everything else
LAYERS = [(64, 48), (32, 40), (64, 64), (64, 56), (128, 128), (144, 64), (256, 128), (64, 128)]
# (B, H, W): below every workgroup threshold, at the 256-workgroup thresholds, above them; odd sizes
MAPS = [(2, 32, 48), (4, 128, 128), (4, 256, 256), (3, 100, 180)]
VARIANT_ALGOS = [None, 'winograd4h', 'direct', 'bf16x3', 'bf16']
POINTWISE = [('plain', 64, 128), ('plainT', 64, 128), ('s2d', 64, 128), ('d2s', 64, 128), ('plain', 32, 64), ('s2d', 24, 40), ('d2s', 48, 16),
             ('plainT', 16, 24)]

LAUNCH_FNS = ('conv3x3', 'conv3x3_winograd', 'conv3x3_winograd_ws', 'conv3x3_winograd4', 'conv3x3_winograd4f', 'conv3x3_winograd4h',
              'conv3x3_winograd4c', 'conv3x3_bf16x3', 'pointwise')
MP_LAUNCH_FNS = ('mp_conv3x3', 'mp_pointwise')
OTHER_OPS_FNS = ('conv3x3_grouped_small',)
OTHER_TOPS_FNS = ('scale_shift_act', 'bn_act_backward', 'colsum', 'conv3x3_wgrad', 'mp_conv3x3_wgrad', 'pointwise_wgrad', 'accumulate')
GROUP_SYMBOLS = ('pcp_pack_conv3x3_group_blocks', 'pcp_pack_conv3x3_group', 'pcp_mp_pack_conv3x3_group_blocks', 'pcp_mp_pack_conv3x3_group')
_DT = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.int16: 'i16', torch.uint8: 'u8', torch.float64: 'f64'}


class Recorder:
    def __init__(self):
        self.calls = []
        self.roles = {}             # data_ptr -> role
        self.keep = []              # every tensor with a role stays alive: its address is never handed out again

    def name_tensor(self, t, role):
        if t is not None:
            self.roles[t.data_ptr()] = role
            self.keep.append(t)

    def role(self, t):
        if type(t) not in (torch.Tensor, nn.Parameter) or t.device.type != 'cpu':
            return None             # a fake or meta tensor has no address
        return self.roles.get(t.data_ptr())

    def ptr_role(self, p):
        return '-' if not p else self.roles.get(p, '?')

    def tensor(self, t):
        return self.role(t) or '%s%s' % (_DT.get(t.dtype, str(t.dtype)), list(t.shape))

    def arg(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, (list, tuple)):
            return '(%s)' % ','.join(self.arg(u) for u in v)
        if v is None or isinstance(v, (bool, int, float, str, torch.dtype)):
            return str(v)
        return type(v).__name__

    def note(self, name, a, k, bias_at=None):
        parts = [self.arg(v) for v in a]
        if bias_at is not None:
            b = a[bias_at]
            real = b.device.type == 'cpu' and type(b) is torch.Tensor
            parts[bias_at] = 'bias%d%s' % (b.numel(), ('+' if bool(b.any()) else '0') if real else '')
        parts += ['%s=%s' % (n, self.arg(k[n])) for n in sorted(k)]
        self.calls.append('%s %s' % (name, ' '.join(parts)))


def _set_algo(value):
    if value is None:
        os.environ.pop('PCP_CONV_ALGO', None)
    else:
        os.environ['PCP_CONV_ALGO'] = value


@contextlib.contextmanager
def _stubs(rec):
    """every launch and packing wrapper the training layers call, replaced on its module; the group repack's library symbols and stream"""
    from pcp_amd import lib, ops, train_ops as tops
    L = lib.load()
    saved = []

    def put(owner, name, fn):
        saved.append((owner, name, getattr(owner, name)))
        setattr(owner, name, fn)

    def launch(name):
        def f(*a, **k):
            rec.note(name, a, k, bias_at=2)
            out = k.get('out')
            if out is None and name.startswith('conv3x3'):          # (x, weights, bias, cin, cout, cout_pad): the launch allocates its output
                (B, H, W, _), st = a[0].shape, k.get('stride', 1)
                out = torch.empty((B, (H - 1) // st + 1, (W - 1) // st + 1, a[4]), dtype=torch.float32, device=a[0].device)
            return out
        return f

    def plain(name):
        def f(*a, **k):
            rec.note(name, a, k)
            return None
        return f

    def bn_train_stats(x, c, gamma, beta, eps, momentum, running_mean, running_var, vec=None, ch_off=0):
        rec.note('bn_train_stats', (x, c, gamma, beta, eps, momentum, running_mean, running_var), dict(vec=vec is not None, ch_off=ch_off))
        return vec if vec is not None else tops.BNVectors(c, x.device)

    def dilate2x(x, c, out=None, ch_off=0):
        rec.note('dilate2x', (x, c), dict(out=out, ch_off=ch_off))
        B, H, W, _ = x.shape
        return out if out is not None else torch.empty((B, 2 * H, 2 * W, c), dtype=x.dtype, device=x.device)

    def rowmap(t, channels, ch_off=0, lattice=None):
        return 'rowmap(%s,%d,%d,%s)' % (rec.tensor(t), channels, ch_off, lattice)

    def side(transpose):
        return 'bw' if transpose else 'fw'

    def pack_conv3x3(w, transpose, direct=None, direct_opad=0, wino=None, wino_opad=0, b3=None, b3_opad=0):
        base = '%s.%s' % (rec.role(w) or '?', side(transpose))
        for t, slot in ((direct, 'direct'), (wino, 'wino'), (b3, 'b3')):
            rec.name_tensor(t, '%s.%s' % (base, slot))
        rec.note('pack_conv3x3', (w, bool(transpose), direct, direct_opad, wino, wino_opad, b3, b3_opad), {})

    def pack_conv3x3_winograd4(w, transpose, u4f=None, u4h=None, opad=0):
        base = '%s.%s' % (rec.role(w) or '?', side(transpose))
        rec.name_tensor(u4f, base + '.f4f')
        rec.name_tensor(u4h, base + '.f4h')
        rec.note('pack_conv3x3_winograd4', (w, bool(transpose), u4f, u4h, opad), {})

    def mp_pack_conv3x3(w, transpose=False, out=None, fold_scale=None):
        cout, cin = int(w.shape[0]), int(w.shape[1])
        K, O = (cout, cin) if transpose else (cin, cout)
        opad = (O + 63) // 64 * 64
        given = out is not None
        if out is None:
            out = torch.empty(K * 9 * opad, dtype=torch.bfloat16, device=w.device)
        rec.name_tensor(out, '%s.%s.mp' % (rec.role(w) or '?', side(transpose)))
        rec.note('mp_pack_conv3x3', (w, bool(transpose)), dict(out_given=given, fold_scale=fold_scale))
        return out, opad

    def blocks(ref):
        j = ref._obj
        return 1 + (j.cout * j.cin) // 2048

    def group_launch(name, struct, fields, ptr_fields):
        def f(table, n, total, stream):
            arr = (struct * n).from_address(table.value)
            jobs = []
            for j in arr:
                jobs.append('[%s %s %s]' % (rec.ptr_role(j.w), ' '.join('%s=%d' % (fl, getattr(j, fl)) for fl in fields),
                                            ' '.join('%s=%s' % (fl, rec.ptr_role(getattr(j, fl))) for fl in ptr_fields)))
            rec.calls.append('%s n=%d total=%d %s' % (name, n, total, ' '.join(jobs)))
            return 0
        return f

    for n in LAUNCH_FNS + OTHER_OPS_FNS:
        put(ops, n, launch(n) if n in LAUNCH_FNS else plain(n))
    for n in MP_LAUNCH_FNS:
        put(tops, n, launch(n))
    for n in OTHER_TOPS_FNS:
        put(tops, n, plain(n))
    for n, fn in (('bn_train_stats', bn_train_stats), ('dilate2x', dilate2x), ('rowmap', rowmap), ('pack_conv3x3', pack_conv3x3),
                  ('pack_conv3x3_winograd4', pack_conv3x3_winograd4), ('mp_pack_conv3x3', mp_pack_conv3x3),
                  ('_stream', lambda: ctypes.c_void_p(0))):
        put(tops, n, fn)
    put(L, GROUP_SYMBOLS[0], blocks)
    put(L, GROUP_SYMBOLS[1], group_launch('pack_conv3x3_group', lib.PackJob,
                                          ('cout', 'cin', 'transpose', 'direct_cout_pad', 'winograd_cout_pad', 'f4_cout_pad', 'block_start'),
                                          ('direct', 'winograd', 'u4f', 'u4h')))
    put(L, GROUP_SYMBOLS[2], blocks)
    put(L, GROUP_SYMBOLS[3], group_launch('mp_pack_conv3x3_group', lib.MpPackJob, ('cout', 'cin', 'transpose', 'out_pad', 'block_start'),
                                          ('packed',)))
    try:
        yield
    finally:
        for owner, name, orig in reversed(saved):
            setattr(owner, name, orig)


@contextlib.contextmanager
def _groups(grouping):
    """fresh group objects and the PCP_PACK_GROUP switch, as module attributes of train_layers (where the layers look them up)"""
    from pcp_amd import train_layers as tl
    saved = (tl.PACK_GROUPING, tl.PACK_GROUP, tl.MP_PACK_GROUP)
    tl.PACK_GROUPING, tl.PACK_GROUP, tl.MP_PACK_GROUP = grouping, tl.tops.PackGroup(), tl.tops.MpPackGroup()
    try:
        yield
    finally:
        tl.flush_batches_tracked()
        tl.PACK_GROUPING, tl.PACK_GROUP, tl.MP_PACK_GROUP = saved


def _conv(kind, cin, cout, stride=1, bias=False, device=None):
    if kind == '3x3':
        return nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=bias, device=device)
    if kind == 'plain':
        return nn.Conv2d(cin, cout, 1, bias=bias, device=device)
    if kind == 's2d':
        return nn.Conv2d(cin, cout, 2, stride=2, bias=bias, device=device)
    return nn.ConvTranspose2d(cin, cout, 2 if kind == 'd2s' else 1, stride=2 if kind == 'd2s' else 1, bias=bias, device=device)


def _layer(rec, tag, kind, cin, cout, stride=1, bias=False, bn=True, device=None, conv=None):
    from pcp_amd import train_layers as tl
    if conv is None:
        conv = _conv(kind, cin, cout, stride, bias, device)
        if rec.role(conv.weight) is None and device is None:
            rec.name_tensor(conv.weight, tag)
    norm = nn.BatchNorm2d(cout, device=device) if bn else None
    return tl.ConvBNAct(conv, norm, relu=bn, name=tag)


def _steps(rec, layers, shapes, algos, in_ld=None, in_off=0, out_ld=None, out_off=0, x_dtype=torch.float32, device='meta', backward_kw=None):
    """one optimizer step per entry of `shapes` / `algos`: tick, forward through the stack, backward through it"""
    from pcp_amd import train_layers as tl
    first, last = layers[0], layers[-1]
    for step, ((B, H, W), algo) in enumerate(zip(shapes, algos)):
        _set_algo(algo)
        rec.calls.append('-- step %d' % step)
        tl.StepClock.tick()
        a = tl.Act(torch.empty((B, H, W, in_ld or first.cin), dtype=x_dtype, device=device), in_off, first.cin)
        for l in layers[:-1]:
            a = l.forward(a)
        out = None
        if out_ld is not None:
            out = tl.Act(torch.empty(last.out_shape(a) + (out_ld,), dtype=torch.float32, device=device), out_off, last.cout)
        y = last.forward(a, out=out)
        rec.calls.append('forward -> %s off=%d c=%d' % (rec.tensor(y.t), y.off, y.c))
        g = tl.Act(torch.empty(tuple(y.t.shape), dtype=y.t.dtype, device=device), y.off, y.c)
        for l in reversed(layers):
            g = l.backward(g, **(backward_kw or {}))
            if g is None:
                break
        rec.calls.append('backward -> %s' % ('None' if g is None else '%s off=%d c=%d' % (rec.tensor(g.t), g.off, g.c)))


def _row(fn, grouping=True):
    rec = Recorder()
    prev = os.environ.get('PCP_CONV_ALGO')
    try:
        with _stubs(rec), _groups(grouping):
            try:
                fn(rec)
            except Exception as e:          # a refusal is part of the behaviour
                rec.calls.append('raised %s: %s' % (type(e).__name__, str(e)[:120]))
    finally:
        _set_algo(prev)
    return rec.calls


def _three(shape, algo):
    return [shape] * 3, [algo] * 3


def record_fake_cuda_rows():
    """the pointwise kinds in the bf16 loop: the bf16 forms are only made for weights on the GPU, so these rows run on fake `cuda` tensors
    (no address: the forms are noted by storage type and shape).  Fake tensors want a process without a GPU: with one, the device index
    must exist and what the layers cache per device would meet the real tensors of other tests"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert not torch.cuda.is_available()
    fake, fake_dev = FakeTensorMode(), 'cuda:7'
    table = {}
    bf16 = torch.bfloat16
    tags = {'bf16 in': dict(x_dtype=bf16), 'f32 in': {}, 'bf16 in at 4': dict(x_dtype=bf16, in_ld=8, in_off=4),
            'bf16 in at 8': dict(x_dtype=bf16, in_ld=8, in_off=8), 'bf16 in, out_off 8': dict(x_dtype=bf16, out_ld=16, out_off=8),
            'bf16 in, out_off 4': dict(x_dtype=bf16, out_ld=16, out_off=4)}

    def row(kind, cin, cout, tag, bias=False, bn=True):
        kw = dict(tags[tag])
        if 'in_ld' in kw:
            kw['in_ld'] += cin
        if 'out_ld' in kw:
            kw['out_ld'] += cout

        def run(rec):
            with fake:
                _steps(rec, [_layer(rec, 'c', kind, cin, cout, 1, bias, bn, device=fake_dev)], *_three((1, 4, 6), 'bf16'), device=fake_dev, **kw)
        table['%s|%d|%d|bf16 on cuda|%s|bias=%d bn=%d' % (kind, cin, cout, tag, bias, bn)] = _row(run)
    for kind, cin, cout in POINTWISE[:4]:
        for tag in ('bf16 in', 'f32 in', 'bf16 in at 4'):
            row(kind, cin, cout, tag)
    for tag in ('bf16 in at 8', 'bf16 in, out_off 8', 'bf16 in, out_off 4'):
        row('plain', 64, 128, tag)
        row('d2s', 64, 128, tag)
    row('plain', 64, 128, 'bf16 in', bias=True, bn=False)
    row('s2d', 64, 128, 'bf16 in', bias=True, bn=False)
    for kind, cin, cout in POINTWISE[4:]:                                    # shapes pcp_mp_pointwise takes in one direction or in none
        row(kind, cin, cout, 'bf16 in')
    return table


def _fake_cuda_rows_from_a_child():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    env.pop('PCP_CONV_ALGO', None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--fake-cuda-rows'], env=env, capture_output=True, text=True, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def record():
    """{row key: [one line per stubbed call, in order]}"""
    table = {}
    big = (4, 128, 128)

    def conv3x3(key, cin, cout, stride, shapes, algos, grouping=True, bias=False, bn=True, **kw):
        table[key] = _row(lambda rec: _steps(rec, [_layer(rec, 'c', '3x3', cin, cout, stride, bias, bn)], shapes, algos, **kw), grouping)

    # the five kinds of launch-time choice.  Every value of the switch on a stride-1, a stride-2 and (the fused forms) a wide layer ...
    sweep = [(64, 64, 1, big, a) for a in ALGOS] + [(64, 128, 2, big, a) for a in ALGOS]
    sweep += [(256, 128, 1, big, a) for a in ('winograd4', 'winograd4f', 'winograd4h', 'winograd4c')]
    sweep += [(64, 64, 1, MAPS[0], a) for a in (None, 'winograd', 'bf16x3', 'winograd4h')]
    # ... every layer at both strides, and in the bf16 loop; the layers around 48 outputs with the split-bf16 kernel asked for ...
    sweep += [(i, o, s, big, None) for i, o in LAYERS for s in (1, 2)] + [(i, o, 1, big, 'bf16') for i, o in LAYERS]
    sweep += [(i, o, 1, big, 'bf16x3') for i, o in LAYERS[:3]]
    # ... and the maps around the workgroup thresholds
    sweep += [(64, 64, 1, m, None) for m in MAPS] + [(256, 128, 1, MAPS[0], None)]
    for cin, cout, stride, shape, algo in dict.fromkeys(sweep):
        conv3x3('3x3|%d|%d|s%d|B%d %dx%d|%s' % ((cin, cout, stride) + shape + (algo,)), cin, cout, stride, *_three(shape, algo))
    # conv bias, BatchNorm and PCP_PACK_GROUP on and off
    for cin, cout, stride, algo in [(64, 64, 1, a) for a in VARIANT_ALGOS] + [(64, 128, 2, None), (64, 56, 1, 'bf16')]:
        for bias in (False, True):
            for bn in (False, True):
                for grouping in (False, True):
                    if algo in (None, 'bf16') and cout == 64 or (bias, bn) in ((False, True), (True, False)):
                        conv3x3('3x3|%d|%d|s%d|%s|bias=%d bn=%d group=%d' % (cin, cout, stride, algo, bias, bn, grouping), cin, cout, stride,
                                *_three(big, algo), grouping=grouping, bias=bias, bn=bn)
    # channel windows: input at an offset that is no multiple of 4 / of 8 / is one, output into a wider buffer, a bf16 input
    bf16 = torch.bfloat16
    windows = {'in_off 2': dict(in_ld=72, in_off=2), 'in_off 4': dict(in_ld=72, in_off=4), 'in_off 8': dict(in_ld=72, in_off=8),
               'in_ld 66': dict(in_ld=66), 'out_off 2': dict(out_ld=72, out_off=2), 'out_off 4': dict(out_ld=72, out_off=4),
               'out_off 8': dict(out_ld=72, out_off=8), 'bf16 in': dict(x_dtype=bf16), 'bf16 in at 4': dict(x_dtype=bf16, in_ld=72, in_off=4),
               'no dx': dict(backward_kw=dict(need_dx=False)), 'accumulate': dict(backward_kw=dict(accumulate=True)),
               'dx f32': dict(backward_kw=dict(dx_dtype=torch.float32))}
    for stride, algo, tags in ((1, None, list(windows)), (1, 'bf16', list(windows)), (1, 'winograd4f', ['in_off 2', 'in_ld 66', 'out_off 2']),
                               (1, 'bf16x3', ['in_off 2', 'in_off 4', 'out_off 4']),
                               (2, None, ['in_off 2', 'out_off 4', 'bf16 in', 'no dx']), (2, 'bf16', ['in_off 4', 'out_off 4', 'dx f32'])):
        for tag in tags:
            conv3x3('3x3|64|64|s%d|%s|%s' % (stride, algo, tag), 64, 64, stride, *_three(big, algo), **windows[tag])
    # the map shape changes between steps (the last partial batch): another fused form, packed and registered again
    for cin, cout, stride, algo in ((64, 64, 1, None), (64, 64, 2, None), (256, 128, 1, None), (64, 64, 1, 'winograd4h'), (64, 64, 1, 'bf16')):
        conv3x3('3x3|%d|%d|s%d|%s|map changes' % (cin, cout, stride, algo), cin, cout, stride,
                [big, big, (1, 128, 128), (1, 128, 128), big], [algo] * 5)
    # PCP_CONV_ALGO changes between steps: the fused choice changes, the group jobs are dropped and registered again
    for seq in (('winograd4f', 'winograd4h', 'direct', 'winograd4h'), (None, None, 'winograd4f', None), ('bf16', 'bf16', None, 'bf16'),
                (None, 'bf16x3', 'bf16x3', None)):
        for grouping in (False, True):
            key = 'stack 64>64 s1, 64>128 s2|%s|group=%d' % ('>'.join(map(str, seq)), grouping)
            table[key] = _row(lambda rec: _steps(rec, [_layer(rec, 'c1', '3x3', 64, 64, 1), _layer(rec, 'c2', '3x3', 64, 128, 2)],
                                                 [(2, 32, 48)] * len(seq), list(seq)), grouping)
        conv3x3('3x3|64|64|s1|%s|group=1' % '>'.join(map(str, seq)), 64, 64, 1, [big] * len(seq), list(seq))

    # two layers sharing one conv module (the weightor runs once per agent): the second application accumulates
    def shared(kind, algo, shape, device):
        def run(rec):
            from pcp_amd import train_layers as tl
            a = _layer(rec, 'c', kind, 64, 64, 1)
            b = _layer(rec, 'c', kind, 64, 64, 1, conv=a.conv)
            for step in range(3):
                _set_algo(algo)
                rec.calls.append('-- step %d' % step)
                tl.StepClock.tick()
                ya = a.forward(tl.Act(torch.empty(shape + (64,), device=device)))
                yb = b.forward(tl.Act(torch.empty(shape + (64,), device=device)))
                a.backward(tl.Act(torch.empty(tuple(ya.t.shape), dtype=ya.t.dtype, device=device)))
                b.backward(tl.Act(torch.empty(tuple(yb.t.shape), dtype=yb.t.dtype, device=device)), accumulate=True)
        return run
    for algo in (None, 'bf16'):
        for grouping in (False, True):
            table['shared 3x3|%s|group=%d' % (algo, grouping)] = _row(shared('3x3', algo, big, 'meta'), grouping)
    table['shared plain|None'] = _row(shared('plain', None, (1, 4, 6), 'cpu'))

    # the four pointwise kinds, on CPU tensors (the weight gradients of the k2 s2 kinds are assembled by torch)
    def pointwise(key, kind, cin, cout, algo, bias=False, bn=True, **kw):
        table[key] = _row(lambda rec: _steps(rec, [_layer(rec, 'c', kind, cin, cout, 1, bias, bn)], *_three((1, 4, 6), algo), device='cpu', **kw))
    variants = ((None, False, True), (None, True, False), (None, True, True), (None, False, False), ('bf16', False, True))
    for n, (kind, cin, cout) in enumerate(POINTWISE):
        for algo, bias, bn in (variants if n < 4 else variants[:1]):         # the narrow shapes: as the layers have them, once
            pointwise('%s|%d|%d|%s|bias=%d bn=%d' % (kind, cin, cout, algo, bias, bn), kind, cin, cout, algo, bias, bn)
    for kind, cin, cout in (POINTWISE[0], POINTWISE[2]):
        for tag, kw in (('in_off 4', dict(in_ld=cin + 8, in_off=4)), ('out_off 8', dict(out_ld=cout + 16, out_off=8)), ('bf16 in', dict(x_dtype=bf16))):
            pointwise('%s|%d|%d|None|%s' % (kind, cin, cout, tag), kind, cin, cout, None, **kw)
    # ... and in the bf16 loop with the weights on the GPU: fake cuda tensors, in a child process that sees no GPU
    table.update(_fake_cuda_rows_from_a_child())

    # the CenterHead branches: stage-1 layers write channel windows of one buffer, ONE data-gradient conv over their gradients
    def head(algo, shape, n, c):
        def run(rec):
            from pcdet.models import train_path
            from pcp_amd import train_layers as tl
            names = ['b%d' % i for i in range(n)]
            h = nn.Module()
            for i, nm in enumerate(names):
                setattr(h, nm, nn.Sequential(nn.Sequential(nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c), nn.ReLU()),
                                             nn.Conv2d(c, 1 + i, 3, padding=1, bias=True)))
                rec.name_tensor(getattr(h, nm)[0][0].weight, nm)
            hb = train_path._HeadBranches(h, names, c)
            for step in range(3):
                _set_algo(algo)
                rec.calls.append('-- step %d' % step)
                tl.StepClock.tick()
                buf = hb.forward(tl.Act(torch.empty(shape + (c,))))
                ds = hb.backward(torch.empty(tuple(buf.shape)))
                rec.calls.append('head backward -> %s' % rec.tensor(ds))
        return run
    for algo in ALGOS:
        table['head 2x64|%s|B2 128x128' % algo] = _row(head(algo, (2, 128, 128), 2, 64))
    table['head 3x32|None|B1 8x16'] = _row(head(None, (1, 8, 16), 3, 32))
    return table


def function_names(table):
    return {line.split(' ')[0] for rows in table.values() for line in rows}


def encode(table):
    """rows are few distinct lines repeated many times: {'codes': [distinct lines], 'rows': {key: [index into codes per line]}}"""
    codes = sorted({r for v in table.values() for r in v})
    at = {c: i for i, c in enumerate(codes)}
    return {'codes': codes, 'rows': {k: [at[r] for r in v] for k, v in table.items()}}


def decode(doc):
    return {k: [doc['codes'][i] for i in v] for k, v in doc['rows'].items()}


if __name__ == '__main__' and sys.argv[1:] == ['--fake-cuda-rows']:
    print(json.dumps(record_fake_cuda_rows()))
elif __name__ == '__main__':
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', '--', 'practical-collab-perception_amd'], cwd=REPO, capture_output=True, text=True).stdout.strip()
    got = record()
    doc = {'recorded_at_commit': commit + (' (with local changes to the package)' if dirty else ''), 'table': encode(got)}
    with open(TABLE, 'w') as f:                              # one code / one row key per line
        f.write(json.dumps(doc, sort_keys=True, separators=(',', ':')).replace('],"', '],\n"').replace('","', '",\n"') + '\n')
    assert json.load(open(TABLE)) == doc
    print('%s: %d rows, %d distinct lines, recorded at %s' % (TABLE, len(got), len(doc['table']['codes']), doc['recorded_at_commit']))
    print(sorted(function_names(got)))
