"""Recorder of the 3x3-conv kernel choice: tests/golden/conv_dispatch_table.json.

Which kernel `PackedConv.run` launches and which fused F(4x4) kernel `train_layers.fused_f4_choice` names are pure host-side decisions, so
they are recorded on the CPU through the public surface only: a layer is packed with `pack_conv_module` / `pack_conv_raw` on CPU tensors, the
`ops.conv3x3*`, `ops.pointwise`, `train_ops.mp_conv3x3` and `train_ops.mp_pointwise` functions are replaced by stubs that note their own name
and the packed form they were handed, and `run` is called on `device='meta'` tensors.  tests/test_host_cpu.py runs `record()` again and
demands equality with the committed file on every row.

The rows put a case on both sides of every comparison of the rule (channel counts around 48 / 128 / 256 / 448 and the 8- / 16- / 32-channel
slices, maps and batches around the 256- and 512-workgroup thresholds, a map that is no multiple of any tile, the over-2-GiB input, unaligned
channel windows and row pitches, every value of PCP_CONV_ALGO plus unset and an unknown one, PCP_WINO4H=0, a bf16 input).

    python tests/golden/make_conv_dispatch_table.py          # rewrites the JSON; the file names the commit it was recorded at
"""
import contextlib
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
TABLE = os.path.join(HERE, 'conv_dispatch_table.json')

ALGOS = [None, 'auto', 'direct', 'winograd', 'winograd4', 'winograd4f', 'winograd4h', 'winograd4c', 'bf16x3', 'bf16', 'no-such-algo']
MAPS = [(16, 16), (64, 64), (128, 128), (256, 256), (100, 180)]
BATCHES = [1, 4, 20, 130]
CINS = [8, 64, 128, 136, 256, 384, 448, 456, 768]
COUTS = [8, 48, 64, 128, 256, 384, 768]
# (cin, cout, stride): the cross product thinned to both sides of every comparison on the layer -- each cin at a narrow, a 128-wide and a
# through-memory-wide output, each cout behind a narrow and a wide input, one cout that is no multiple of 4, stride 2 at each width class.
# pack_conv3x3 takes multiples of 16 input channels only (8, 136 and 456 are recorded as refused), so 16, 144 and 464 stand on the far side
# of the 128- and 448-channel comparisons; 144 is also no multiple of the through-memory form's 32-channel slice
LAYERS = sorted({(ci, co, 1) for ci in CINS + [16, 144, 464] for co in (48, 128, 256)} | {(ci, co, 1) for ci in (64, 128, 464) for co in COUTS}
                | {(768, 768, 1), (384, 384, 1), (64, 50, 1), (16, 8, 2), (64, 64, 2), (128, 256, 2), (464, 128, 2), (768, 768, 2)})
RAW_LAYERS = [(64, 64, 1), (128, 256, 1), (384, 128, 1), (768, 768, 1), (64, 128, 2)]          # pack_conv_raw (the CenterHead branches)
POINTWISE = [('plain', 64, 128), ('s2d', 64, 64), ('d2s', 128, 64), ('plainT', 64, 64)]
CONV_FNS = ('conv3x3', 'conv3x3_winograd', 'conv3x3_winograd_ws', 'conv3x3_winograd4', 'conv3x3_winograd4f', 'conv3x3_winograd4h',
            'conv3x3_winograd4c', 'conv3x3_bf16x3', 'pointwise')
MP_FNS = ('mp_conv3x3', 'mp_pointwise')


def launches(cin, cout, stride):
    """(label, B, H, W, ld_in, in_ch_off, out ld | None = allocated by the launch, out_ch_off, input dtype) of one layer"""
    rows = [('B%d %dx%d' % (B, H, W), B, H, W, cin, 0, None, 0, 'f32') for (H, W) in MAPS for B in BATCHES]
    for B, H, W in ((4, 256, 256), (20, 64, 64), (20, 128, 128)):
        t = 'B%d %dx%d ' % (B, H, W)
        rows += [(t + 'in_ch_off 2', B, H, W, cin + 4, 2, None, 0, 'f32'), (t + 'in_ch_off 4', B, H, W, cin + 4, 4, None, 0, 'f32'),
                 (t + 'ld_in % 4 = 2', B, H, W, cin + 2, 0, None, 0, 'f32'), (t + 'out ld % 4 = 2', B, H, W, cin, 0, cout + 2, 0, 'f32'),
                 (t + 'out_ch_off 2', B, H, W, cin, 0, cout + 4, 2, 'f32'), (t + 'out_ch_off 4', B, H, W, cin, 0, cout + 4, 4, 'f32'),
                 (t + 'bf16 in, window at 2', B, H, W, cin + 2, 2, None, 0, 'bf16')]
    return rows


@contextlib.contextmanager
def _algo(value):
    prev = os.environ.get('PCP_CONV_ALGO')
    if value is None:
        os.environ.pop('PCP_CONV_ALGO', None)
    else:
        os.environ['PCP_CONV_ALGO'] = value
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop('PCP_CONV_ALGO', None)
        else:
            os.environ['PCP_CONV_ALGO'] = prev


def _constants_home():
    """the module that holds the dispatch thresholds (pcdet/models/convnet.py at the commit the table was recorded at)"""
    try:
        from pcp_amd import conv_dispatch
        return conv_dispatch
    except ImportError:
        from pcdet.models import convnet
        return convnet


@contextlib.contextmanager
def _wino4h(value):
    home = _constants_home()
    prev = home.WINOGRAD4H
    home.WINOGRAD4H = value
    try:
        yield
    finally:
        home.WINOGRAD4H = prev


@contextlib.contextmanager
def _stubs(calls):
    from pcp_amd import ops, train_ops
    saved = [(m, n, getattr(m, n)) for m, names in ((ops, CONV_FNS), (train_ops, MP_FNS)) for n in names]

    def stub(name):
        def f(*a, **k):
            calls.append((name, a, k))
            return None
        return f
    for m, n, _ in saved:
        setattr(m, n, stub(n))
    try:
        yield
    finally:
        for m, n, orig in saved:
            setattr(m, n, orig)


def _describe(pc, call):
    """'function/packed form/cout_pad/in_ch_off[/plain]' of one stubbed launch"""
    name, a, k = call
    forms = {id(getattr(pc, s)[0]): s for s in ('wino', 'b3', 'w4', 'w4f', 'w4h', 'w4c', 'mp') if getattr(pc, s, None) is not None}
    forms[id(pc.w)] = 'w'
    cout_pad = a[6] if name in ('pointwise', 'mp_pointwise') else a[5]
    s = '%s/%s/%d/%d' % (name, forms.get(id(a[1]), '?'), cout_pad, k['in_ch_off'])
    return s + '/plain' if k.get('plain') else s


def _run_rows(pc, rows, stride=1):
    got = []
    for (_label, B, H, W, ld_in, in_off, out_ld, out_off, dt) in rows:
        x = torch.empty((B, H, W, ld_in), dtype=torch.bfloat16 if dt == 'bf16' else torch.float32, device='meta')
        out = None
        if out_ld is not None:
            out = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, out_ld), dtype=torch.float32, device='meta')
        calls = []
        with _stubs(calls):
            pc.run(x, out=out, in_ch_off=in_off, out_ch_off=out_off)
        assert len(calls) == 1, calls
        got.append(_describe(pc, calls[0]))
    return got


def _layer(kind, cin, cout, stride):
    if kind == '3x3':
        return nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
    if kind == 'plain':
        return nn.Conv2d(cin, cout, 1, bias=False)
    if kind == 's2d':
        return nn.Conv2d(cin, cout, 2, stride=2, bias=False)
    return nn.ConvTranspose2d(cin, cout, 2 if kind == 'd2s' else 1, stride=2 if kind == 'd2s' else 1, bias=False)


def record_dispatch():
    """{'pack algo>run algo|cin|cout|stride|packer[|PCP_WINO4H=0]': [one launch description per row of launches()]}: every layer packed and run
    under each value of the switch, and packed with the switch unset but run under each value (a model that is not repacked after a change)"""
    from pcdet.models import convnet
    table = {}
    torch.manual_seed(0)
    jobs = [('module', l) for l in LAYERS] + [('raw', l) for l in RAW_LAYERS]
    for packer, (cin, cout, stride) in jobs:
        rows = launches(cin, cout, stride)
        conv = _layer('3x3', cin, cout, stride)
        for pack_algo in ALGOS:
            with _algo(pack_algo):
                try:
                    if packer == 'module':
                        pc = convnet.pack_conv_module(conv, None, relu=True)
                    else:
                        pc = convnet.pack_conv_raw(conv.weight.detach(), torch.zeros(cout), relu=True, stride=stride)
                except AssertionError:
                    table['%s|%d|%d|%d|%s' % (pack_algo, cin, cout, stride, packer)] = 'refused by pack_conv3x3'
                    continue
            for run_algo in (ALGOS if pack_algo is None else [pack_algo]):
                key = '%s>%s|%d|%d|%d|%s' % (pack_algo, run_algo, cin, cout, stride, packer)
                with _algo(run_algo):
                    table[key] = _run_rows(pc, rows, stride)
                    if run_algo in (None, 'winograd4h', 'winograd4c'):
                        with _wino4h('0'):
                            table[key + '|PCP_WINO4H=0'] = _run_rows(pc, rows, stride)
    for kind, cin, cout in POINTWISE:
        for algo in (None, 'bf16'):
            with _algo(algo):
                pc = convnet.pack_conv_module(_layer(kind, cin, cout, 1), None, relu=False)
                table['%s>%s|%d|%d|%s' % (algo, algo, cin, cout, kind)] = _run_rows(pc, launches(cin, cout, 1)[:4])
    return table


F4_CODE = {None: '-', '4f': 'f', '4h': 'h'}


def f4_launches():
    return [(B, H, W) for (H, W) in MAPS for B in BATCHES]


def record_fused_f4():
    """{'algo|cin|cout[|PCP_WINO4H=0]': one character per f4_launches() row: - (neither), f (k_wino4f), h (k_wino4h)}"""
    from pcp_amd import train_layers
    table = {}
    for algo in ALGOS:
        for cin in CINS + [12]:
            for cout in COUTS + [50]:
                with _algo(algo):
                    table['%s|%d|%d' % (algo, cin, cout)] = ''.join(F4_CODE[train_layers.fused_f4_choice(B, H, W, cin, cout)] for B, H, W in f4_launches())
                    if algo is None:
                        with _wino4h('0'):
                            table['%s|%d|%d|PCP_WINO4H=0' % (algo, cin, cout)] = ''.join(
                                F4_CODE[train_layers.fused_f4_choice(B, H, W, cin, cout)] for B, H, W in f4_launches())
    return table


def record():
    return {'dispatch': record_dispatch(), 'fused_f4_choice': record_fused_f4()}


def encode(table):
    """rows are few distinct strings repeated many times: {'codes': [distinct rows], 'rows': {key: [index into codes per launch]}}"""
    codes = sorted({r for v in table.values() if isinstance(v, list) for r in v})
    at = {c: i for i, c in enumerate(codes)}
    return {'codes': codes, 'rows': {k: ([at[r] for r in v] if isinstance(v, list) else v) for k, v in table.items()}}


def decode(doc):
    return {k: ([doc['codes'][i] for i in v] if isinstance(v, list) else v) for k, v in doc['rows'].items()}


if __name__ == '__main__':
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', '--', 'practical-collab-perception_amd'], cwd=REPO, capture_output=True, text=True).stdout.strip()
    got = record()
    doc = {'recorded_at_commit': commit + (' (with local changes to the package)' if dirty else ''),
           'launches': [r[0] for r in launches(64, 64, 1)], 'fused_f4_launches': ['B%d %dx%d' % l for l in f4_launches()],
           'dispatch': encode(got['dispatch']), 'fused_f4_choice': got['fused_f4_choice']}
    with open(TABLE, 'w') as f:                              # one table key per line
        f.write(json.dumps(doc, sort_keys=True, separators=(',', ':')).replace('],"', '],\n"').replace('","', '",\n"') + '\n')
    assert json.load(open(TABLE)) == doc
    print('%s: %d dispatch keys, %d fused_f4_choice keys, recorded at %s' % (TABLE, len(got['dispatch']), len(got['fused_f4_choice']), doc['recorded_at_commit']))
