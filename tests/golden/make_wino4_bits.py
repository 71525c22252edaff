"""Recorder of the output BITS of the fused F(4x4, 3x3) kernels: tests/golden/wino4_bits.json.

k_wino4f, k_wino4h and k_wino4c (csrc/wino4f.hip, wino4h.hip, wino4c.hip) are run through `pcp_amd.ops` on weights packed by `pcp_amd.pack`;
inputs, weights and biases are drawn on the CPU the way tests/test_gpu_ops.py::_rand draws them.  For every launch the JSON holds the SHA-256
of the output tensor's bytes.  tests/test_gpu_wino4_bits.py runs `record()` again and demands equality with the committed file, so a kernel
change that claims "bit-identical" is checked against the commit the file was recorded at, not against another kernel of the same build.

Cases (cin, cout, h, w, batch), the smallest shapes at which each mechanism can break:
    (8, 64, 16, 32, 1)       one slice: prologue and last step only
    (24, 128, 7, 9, 1)       three slices; a map smaller than one item; both ragged edges
    (64, 100, 20, 36, 2)     padded cout; ragged; two frames
    (384, 64, 16, 32, 1)     48 slices
    (64, 384, 33, 47, 1)     cout_pad % 128 == 0: k_wino4c's 64-channel form (wino4c_nw 4) and its 128-channel form (wino4c_nw 8)
    (72, 132, 20, 100, 3)    cout_pad 192: with wino4c_nw 8 k_wino4c falls back to the 64-channel form
each with and without ReLU, plus the channel-window launch of test_conv3x3_winograd4f_channel_windows_and_bad_arguments (the whole pre-filled
buffer is hashed).

Record with the library of the commit whose bits are to be pinned (PCP_HIP_LIB selects a library built elsewhere):
    PCP_HIP_LIB=<parent build>/libpcp_hip.so python tests/golden/make_wino4_bits.py --commit <hash of that commit>
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, 'practical-collab-perception_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
TABLE = os.path.join(HERE, 'wino4_bits.json')

CASES = [(8, 64, 16, 32, 1), (24, 128, 7, 9, 1), (64, 100, 20, 36, 2), (384, 64, 16, 32, 1), (64, 384, 33, 47, 1), (72, 132, 20, 100, 3)]
KERNELS = ['winograd4f', 'winograd4h', 'winograd4c']


def _rand(seed, shape, lo=-1.0, hi=1.0):
    from pcp_amd import synth
    return synth.uniform(seed, 5, int(np.prod(shape)), lo, hi).reshape(shape)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _forms(kernel):
    """the launches of one kernel: (key suffix, wino4c_nw or None)"""
    return [('|nw4', 4), ('|nw8', 8)] if kernel == 'winograd4c' else [('', None)]


def record(set_option):
    """key -> SHA-256 of the output bytes.  set_option(name, value) sets a library option (the tests pass the lib_option fixture)."""
    from pcp_amd import ops, pack
    d = torch.device('cuda:0')
    got = {}
    for cin, cout, h, w, batch in CASES:
        x = ops.as_nhwc(torch.from_numpy(_rand(291, (batch, cin, h, w))).to(d))
        wt = torch.from_numpy(_rand(292, (cout, cin, 3, 3), -0.05, 0.05))
        b = torch.from_numpy(_rand(293, (cout,), -0.2, 0.2))
        for kernel in KERNELS:
            packed, bp, cpad = getattr(pack, 'pack_conv3x3_' + kernel)(wt, b)
            packed, bp = packed.to(d), bp.to(d)
            for suffix, nw in _forms(kernel):
                if nw is not None:
                    set_option('wino4c_nw', nw)
                for relu in (False, True):
                    out = getattr(ops, 'conv3x3_' + kernel)(x, packed, bp, cin, cout, cpad, relu=relu)
                    got['%s|%d,%d,%d,%d,%d|relu%d%s' % (kernel, cin, cout, h, w, batch, relu, suffix)] = _sha(out)
    # channel windows: 64 of 96 input channels from offset 16, 128 output channels at offset 128 of a pre-filled 384-channel buffer
    cin, cout = 64, 128
    wt = torch.from_numpy(_rand(277, (cout, cin, 3, 3), -0.05, 0.05))
    x = torch.from_numpy(_rand(278, (1, 48, 40, 96))).to(d)
    for kernel in KERNELS:
        packed, bp, cpad = getattr(pack, 'pack_conv3x3_' + kernel)(wt, torch.zeros(cout))
        for suffix, nw in _forms(kernel):
            if nw is not None:
                set_option('wino4c_nw', nw)
            out = torch.full((1, 48, 40, 384), 7.0, device=d)
            getattr(ops, 'conv3x3_' + kernel)(x, packed.to(d), bp.to(d), cin, cout, cpad, relu=False, out=out, in_ch_off=16, out_ch_off=128)
            got['%s|window%s' % (kernel, suffix)] = _sha(out)
    torch.cuda.synchronize()
    return got


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the loaded library was built from')
    ap.add_argument('--out', default=TABLE)
    args = ap.parse_args()
    from pcp_amd import lib
    doc = {'recorded_at_commit': args.commit, 'sha256': record(lib.set_option)}
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%s: %d launches of the library %s, recorded at %s' % (args.out, len(doc['sha256']), lib.LIB_PATH, args.commit))
