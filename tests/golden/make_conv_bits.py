"""Recorder of the output BITS of the convolution and weight-gradient kernels outside the fused F(4x4) family: tests/golden/conv_bits.json.

These kernels share the XCD workgroup remap and the fp32 MFMA wrapper of csrc/pcp_common.h and, the two pointwise weight gradients, the
row map and the split-K reduce of csrc/splitk_common.h.  Their other tests compare with a reference inside a tolerance; this file pins
every launch to the SHA-256 of its output bytes at the commit the JSON names, so a change that claims "same code" is held to it.
tests/test_gpu_conv_bits.py runs `record()` again and demands equality with the committed file.  Every launch runs TWICE and the two
hashes must agree (the split-K reduces sum in a fixed order: DESIGN section 5).

Inputs are seeded integers scaled by a power of two (fp32: |i| <= 1000 / 1024, weights |i| <= 100 / 2048; bf16 operands |i| <= 127 / 128,
exact in bf16): exact to write down, wide enough that the sums round, so another summation order gives other bits.

Maps (B, H, W): N = (3, 48, 40) and M = (2, 32, 64).  With the smallest channel counts an entry point takes, every kernel that maps
blockIdx through xcd_remap gets a grid that is NOT a multiple of 8 workgroups on N (the remainder branch) and one that is on M:
    pcp_conv3x3 s1 (8 x 16 pixels x 64 or 32 channels)              54 | 32
    pcp_conv3x3 s2, cout_pad 32 (8 x 16)                            18 |  8
    pcp_conv3x3 s2, conv_s2_form 1 (8 x 8 x 64)                     27 | 16
    pcp_conv3x3 s2, conv_s2_form 2 (8 x 16 x 64 | 8 x 8 x 128)      18 |  8,  27 | 16
    pcp_pointwise PLAIN / SPACE2DEPTH / DEPTH2SPACE (128 rows x 64) 45 | 32,  12 |  8,  180 | 128
    pcp_conv3x3_winograd RT 1 (8 x 16 x 64)                         54 | 32
    pcp_conv3x3_winograd RT 2 (16 x 16 x 64; needs cin >= 256 and >= 256 workgroups: cout 640 on N, 1024 on M)   270 | 256
    pcp_conv3x3_winograd_ws (8 x 16 x 64)                           54 | 32
    pcp_conv3x3_bf16x3 / _bf16 s1 (16 x 16 x 64), s2 (8 x 16 x 64)  27 | 16,  18 |  8
    pcp_mp_conv3x3 fast kernel (8 x 32 x 64 items, one workgroup each below the CU count), general kernel at s2 (8 x 16 x 64)   36 | 16,  18 | 8
    pcp_mp_conv3x3_wgrad s1 / s2 (64 -> 64: batch x strips x row splits)     36 | 16,  18 | 8
    pcp_mp_pointwise, three modes (128 rows x 64)                   as pcp_pointwise
    pcp_hunter_point_head with an `order` (32 points)               379 points: 12 | 512 points: 16
pcp_conv3x3_winograd4 (its GEMM deals tiles to persistent workgroups itself) runs on both maps as well.

Weight gradients:
    pcp_pointwise_wgrad     300 rows (three 128-row chunks, ragged tail) x (32, 16) one quadrant, (64, 32) two quadrants, (96, 64) two tiles;
                            (64, 32) on lattice row maps over a 6 x 10 grid, (ky, kx) = (1, 0) and (0, 1); accumulate 0 and 1; the output is a
                            window of a wider buffer, which is hashed whole
    pcp_mp_pointwise_wgrad  1000 rows (32 stages, four splits) x (64, 32), (96, 64); the same lattice (1020 rows); accumulate 0 and 1
    pcp_conv3x3_wgrad       stride 1 and 2, 16 -> 32 and 64 -> 96, (2, 16, 24)

Record with the library of the commit whose bits are to be pinned (PCP_HIP_LIB selects a library built elsewhere):
    PCP_HIP_LIB=<parent build>/libpcp_hip.so python tests/golden/make_conv_bits.py --commit <hash of that commit>
"""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, 'practical-collab-perception_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
TABLE = os.path.join(HERE, 'conv_bits.json')

MAPS = [(3, 48, 40), (2, 32, 64)]
LATTICE = (6, 10)


def _ints(seed, shape, bound, shift):
    """seeded integers of [-bound, bound] times 2^-shift, float32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, tuple(shape), generator=g).float() * (2.0 ** -shift)


def _x(seed, shape):
    return _ints(seed, shape, 1000, 10)


def _w(seed, shape):
    return _ints(seed, shape, 100, 11)


def _b16(seed, shape):
    return _ints(seed, shape, 127, 7)


def _sha(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


class _Table(dict):
    def run(self, key, launch):
        """launch() -> the tensor to hash; run twice, the two hashes must agree"""
        first, second = _sha(launch()), _sha(launch())
        assert first == second, '%s: two runs of one launch gave different bits' % key
        assert key not in self, key
        self[key] = first


def _mapkey(m):
    return '%d,%d,%d' % m


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv_family(got, set_option, d):
    from pcp_amd import lib, ops, pack
    for m in MAPS:
        B, H, W = m
        mk = _mapkey(m)
        x = {c: _nhwc(_x(11 + c, (B, c, H, W))).to(d) for c in (8, 16, 32, 256)}

        def weights(cin, cout, packer, seed=21):
            wt, b = _w(seed + cin + cout, (cout, cin, 3, 3)), _w(seed + 1 + cout, (cout,))
            packed, bp, cpad = packer(wt, b)
            return packed.to(d), bp.to(d), cpad

        # direct fp32: stride 1 (64- and 32-channel tiles), stride 2 (32-channel tile; both forms of the 64-channel one; the 128-channel wide form)
        for cout in (64, 32):
            p, bp, cpad = weights(16, cout, pack.pack_conv3x3)
            got.run('conv3x3|s1|16,%d|%s' % (cout, mk), lambda: ops.conv3x3(x[16], p, bp, 16, cout, cpad, stride=1, relu=True))
        p, bp, cpad = weights(16, 32, pack.pack_conv3x3)
        got.run('conv3x3|s2|16,32|%s' % mk, lambda: ops.conv3x3(x[16], p, bp, 16, 32, cpad, stride=2, relu=True))
        for form, cout in ((1, 64), (2, 64), (2, 128)):
            set_option('conv_s2_form', form)
            p, bp, cpad = weights(16, cout, pack.pack_conv3x3)
            got.run('conv3x3|s2 form %d|16,%d|%s' % (form, cout, mk), lambda: ops.conv3x3(x[16], p, bp, 16, cout, cpad, stride=2, relu=False))
        set_option('conv_s2_form', None)

        # pointwise, three modes
        for mode, name, packer, wshape in ((lib.PW_PLAIN, 'plain', pack.pack_plain, (64, 16)),
                                           (lib.PW_SPACE2DEPTH, 'space2depth', pack.pack_conv2x2_s2, (64, 16, 2, 2)),
                                           (lib.PW_DEPTH2SPACE, 'depth2space', pack.pack_convT2x2_s2, (16, 64, 2, 2))):
            packed, bp, cpad = packer(_w(31 + mode, wshape), _w(35 + mode, (64,)))
            packed, bp = packed.to(d), bp.to(d)
            got.run('pointwise|%s|16,64|%s' % (name, mk), lambda: ops.pointwise(x[16], packed, bp, mode, 16, 64, cpad, relu=True))

        # fused F(2x2): 32-tile workgroups (RT 1), 64-tile workgroups (RT 2), the wave-stationary form
        p, bp, cpad = weights(8, 64, pack.pack_conv3x3_winograd)
        got.run('winograd|rt1|8,64|%s' % mk, lambda: ops.conv3x3_winograd(x[8], p, bp, 8, 64, cpad, relu=True))
        cout = 640 if B == 3 else 1024
        p, bp, cpad = weights(256, cout, pack.pack_conv3x3_winograd)
        got.run('winograd|rt2|256,%d|%s' % (cout, mk), lambda: ops.conv3x3_winograd(x[256], p, bp, 256, cout, cpad, relu=True))
        p, bp, cpad = weights(32, 64, pack.pack_conv3x3_winograd_ws)
        got.run('winograd_ws|32,64|%s' % mk, lambda: ops.conv3x3_winograd_ws(x[32], p, bp, 32, 64, cpad, relu=True))
        # F(4x4) through memory
        p, bp, cpad = weights(32, 64, pack.pack_conv3x3_winograd4)
        got.run('winograd4|32,64|%s' % mk, lambda: ops.conv3x3_winograd4(x[32], p, bp, 32, 64, cpad, relu=True))
        # bf16 products on fp32 maps: split (bf16x3) and plain
        p, bp, cpad = weights(16, 64, pack.pack_conv3x3_bf16x3)
        for stride in (1, 2):
            for plain in (False, True):
                got.run('%s|s%d|16,64|%s' % ('bf16' if plain else 'bf16x3', stride, mk),
                        lambda: ops.conv3x3_bf16x3(x[16], p, bp, 16, 64, cpad, stride=stride, relu=True, plain=plain))


def _mp_family(got, d):
    from pcp_amd import lib, pack, train_ops as tops
    for m in MAPS:
        B, H, W = m
        mk = _mapkey(m)
        xb = {c: _nhwc(_b16(41 + c, (B, c, H, W))).to(d).to(torch.bfloat16) for c in (16, 32, 64)}
        # the fast kernel (stride 1, bf16 input, cin % 32 == 0) and the general one (stride 2)
        for name, cin, stride in (('fast', 32, 1), ('general', 16, 2)):
            packed, opad = tops.mp_pack_conv3x3(_w(51 + cin, (64, cin, 3, 3)).to(d))
            bias = _w(53, (opad,)).to(d)
            got.run('mp_conv3x3|%s|%d,64|%s' % (name, cin, mk), lambda: tops.mp_conv3x3(xb[cin], packed, bias, cin, 64, opad, stride=stride, relu=True))
        for stride in (1, 2):
            dy = _nhwc(_b16(55 + stride, (B, 64, H // stride, W // stride))).to(d).to(torch.bfloat16)

            def wgrad():
                dw = torch.full((64, 64, 3, 3), 5.0, device=d)
                return tops.mp_conv3x3_wgrad(xb[64], dy, 64, 64, stride, dw)
            got.run('mp_conv3x3_wgrad|s%d|64,64|%s' % (stride, mk), wgrad)
        for mode, name, packer, wshape in ((lib.PW_PLAIN, 'plain', pack.pack_plain, (64, 32)),
                                           (lib.PW_SPACE2DEPTH, 'space2depth', pack.pack_conv2x2_s2, (64, 32, 2, 2)),
                                           (lib.PW_DEPTH2SPACE, 'depth2space', pack.pack_convT2x2_s2, (32, 64, 2, 2))):
            packed, bp, cpad = packer(_b16(61 + mode, wshape), _w(65 + mode, (64,)))
            packed, bp = packed.to(d).to(torch.bfloat16), bp.to(d)
            got.run('mp_pointwise|%s|32,64|%s' % (name, mk), lambda: tops.mp_pointwise(xb[32], packed, bp, mode, 32, 64, cpad, relu=True))


def _point_head(got, d):
    from pcp_amd import ops
    C, B, H, W = 384, 2, 16, 24
    bev = _nhwc(_x(71, (B, C, H, W))).to(d)
    wts = [t.to(d) for t in (_w(72, (32, C)), _w(73, (32,)), _w(74, (C, 32)), _w(75, (C,)), _w(76, (8, C)), _w(77, (8,)))]
    for n in (379, 512):
        g = torch.Generator().manual_seed(78 + n)
        pts = torch.zeros((n, 5))
        pts[:, 0] = torch.randint(0, B, (n,), generator=g).float()
        pts[:, 1] = torch.randint(-64, W * 32 + 64, (n,), generator=g).float() / 32.0        # pixel units 1 x 1 from the origin; some rows outside
        pts[:, 2] = torch.randint(-64, H * 32 + 64, (n,), generator=g).float() / 32.0
        order = torch.randperm(n, generator=g).to(torch.int32).to(d)
        pts = pts.to(d)

        def launch():
            pf, head = ops.hunter_point_head(bev, pts, [0.0, 0.0], [1.0, 1.0], *wts, channels=C, order=order)
            return torch.cat([pf, head], 1)
        got.run('point_head|order|%d' % n, launch)


def _pointwise_wgrads(got, d):
    from pcp_amd import train_ops as tops
    gh, gw = LATTICE
    for name, rows, lat_b, pairs, draw, dt in (('pointwise_wgrad', 300, 5, [(32, 16), (64, 32), (96, 64)], _x, torch.float32),
                                               ('mp_pointwise_wgrad', 1000, 17, [(64, 32), (96, 64)], _b16, torch.bfloat16)):
        cases = [(n, k, None) for n, k in pairs] + [(64, 32, lat_b)]
        for n, k, lb in cases:
            if lb is None:
                a, b = draw(81 + n, (rows, n)).to(d).to(dt), draw(82 + k, (rows, k)).to(d).to(dt)
                ma, mb, r = tops.rowmap(a, n), tops.rowmap(b, k), rows
            else:
                a, b = draw(83, (lb, 2 * gh, 2 * gw, n)).to(d).to(dt), draw(84, (lb, 2 * gh, 2 * gw, k)).to(d).to(dt)
                ma, mb, r = tops.rowmap(a, n, lattice=(gh, gw, 1, 0)), tops.rowmap(b, k, lattice=(gh, gw, 0, 1)), lb * gh * gw
            for acc in (0, 1):
                def launch():
                    buf = _x(85, (n, k + 8)).to(d)                   # the output is the window [4, 4 + k) of these rows
                    tops.pointwise_wgrad(ma, mb, r, buf[:, 4:4 + k], accumulate=bool(acc))
                    return buf
                got.run('%s|%d,%d|%s|acc%d' % (name, n, k, 'rows %d' % r if lb is None else 'lattice %dx%d rows %d' % (gh, gw, r), acc), launch)


def _conv_wgrad(got, d):
    from pcp_amd import train_ops as tops
    B, H, W = 2, 16, 24
    for cin, cout in ((16, 32), (64, 96)):
        x = _nhwc(_x(91 + cin, (B, cin, H, W))).to(d)
        for stride in (1, 2):
            dy = _nhwc(_x(92 + cout + stride, (B, cout, H // stride, W // stride))).to(d)

            def launch():
                dw = torch.full((cout, cin, 3, 3), 5.0, device=d)
                return tops.conv3x3_wgrad(x, dy, cin, cout, stride, dw)
            got.run('conv3x3_wgrad|s%d|%d,%d|%d,%d,%d' % (stride, cin, cout, B, H, W), launch)


def record(set_option):
    """key -> SHA-256 of the output bytes.  set_option(name, value) sets a library option (the tests pass the lib_option fixture)."""
    d = torch.device('cuda:0')
    got = _Table()
    _conv_family(got, set_option, d)
    _mp_family(got, d)
    _point_head(got, d)
    _pointwise_wgrads(got, d)
    _conv_wgrad(got, d)
    torch.cuda.synchronize()
    return dict(got)


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
