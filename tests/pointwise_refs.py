"""Plain float64 references (numpy, no GPU) of the fp32 pointwise family and its weight gradient, the error bound their tests use as
tolerance, and the case tables those tests share.

  plain, space2depth, depth2space   pcp_pointwise, modes PW_PLAIN / PW_SPACE2DEPTH / PW_DEPTH2SPACE        (csrc/conv.hip, k_pointwise)
  pw_wgrad                          pcp_pointwise_wgrad with the row maps of include/pcp_hip_train.h        (csrc/wgrad.hip, k_wgrad_pw)

Maps are NHWC arrays ((rows, C) for the plain mode); weights have torch's layouts: Linear / 1x1 (cout, cin), Conv2d k2 s2
(cout, cin, 2, 2), ConvTranspose2d k2 s2 (cin, cout, 2, 2).  Float32 inputs enter the arithmetic as their exact float64 values.

The bound.  An fp32 sum of K products, in any order and with or without fused multiply-adds, differs from the exact value by at most
(K + 2) * 2^-24 * S, where S = sum_k |x_k| |w_k| + |b| + |residual| (every one of the K multiplications and of the K + 1 additions rounds
once, relative error 2^-24 each, and a term passes through at most K + 2 of them; the second-order terms are below 2^-24 of the bound for
every K used here).  Every reference returns S next to its result; bound(S, K) is the tolerance, element by element and with nothing on
top.  Where a ReLU follows, the bound of the value before the clamp holds after it: relu is 1-Lipschitz.  For the weight gradient K is the
row count: the split-K partial sums and their reduction are additions of the same sum.
"""
import functools
from collections import namedtuple

import numpy as np

from pcp_amd import synth

U = 2.0 ** -24
CK = 16                  # input channels per staged slice (csrc/conv.hip)
BM = 128                 # rows per workgroup of k_pointwise
PW_ROWS = 128            # rows per chunk of k_wgrad_pw


def f64(x):
    return np.asarray(x, dtype=np.float64)


def bound(S, K):
    return (K + 2) * U * S


def uniform(seed, col, shape, lo=-1.0, hi=1.0):
    n = int(np.prod(shape))
    return synth.uniform(7300 + seed, col, n, lo, hi).reshape(shape).astype(np.float32)


def small_ints(seed, col, shape):
    """non-zero integers in [-16, 16] as float32: sums of one of them and zeros are exact, and no signed zero can arise"""
    mag = np.floor(f64(uniform(seed, col, shape, 1.0, 17.0)))
    sign = np.where(uniform(seed, col + 1, shape) < 0, -1.0, 1.0)
    return (np.clip(mag, 1, 16) * sign).astype(np.float32)


def cout_pad_of(cout):
    """pack.py's rule, restated: 32 up to 32 output channels (the 128x32 instantiation), multiples of 64 above (128x64)"""
    return 32 if cout <= 32 else (cout + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------------
# forward references
# ---------------------------------------------------------------------------------------------------------------------

def finish(acc, S, b, residual=None, relu=False, residual_before_relu=False):
    """bias, activation and residual of the epilogue on the contraction `acc` (S = its sum of absolute products): (y, S)"""
    y = acc + f64(b)
    S = S + np.abs(f64(b))
    if residual is not None:
        S = S + np.abs(f64(residual))
    if residual_before_relu:
        assert residual is not None and relu
        y = np.maximum(y + f64(residual), 0.0)
    else:
        if relu:
            y = np.maximum(y, 0.0)
        if residual is not None:
            y = y + f64(residual)
    return y, S


def plain_acc(x, w, x2=None, k_split=0):
    """sum_k xcat[r, k] w[n, k] and sum_k |.||.|; with x2, contraction channels [k_split, cin) come from x2[:, k - k_split]"""
    x, w = f64(x), f64(w)
    if x2 is None:
        return x @ w.T, np.abs(x) @ np.abs(w).T
    x2 = f64(x2)
    assert x.shape[-1] == k_split and k_split + x2.shape[-1] == w.shape[1]
    acc = x @ w[:, :k_split].T + x2 @ w[:, k_split:].T
    S = np.abs(x) @ np.abs(w[:, :k_split]).T + np.abs(x2) @ np.abs(w[:, k_split:]).T
    return acc, S


def plain(x, w, b, x2=None, k_split=0, residual=None, relu=False, residual_before_relu=False):
    """x (rows, cin) [or (rows, k_split) with x2 (rows, cin - k_split)], w (cout, cin), b (cout,), residual (rows, cout) -> (y, S)"""
    acc, S = plain_acc(x, w, x2, k_split)
    return finish(acc, S, b, residual, relu, residual_before_relu)


def tap_pixels(x, ky, kx):
    """the pixels (b, 2y + ky, 2x + kx) of an NHWC map, as a (B, H/2, W/2, C) view"""
    return x[:, ky::2, kx::2, :]


def space2depth_taps(x, w):
    """the four tap terms of Conv2d(k2, s2): [(acc, S)] in tap order ky * 2 + kx, each (B, H/2, W/2, cout)"""
    x, w = f64(x), f64(w)
    out = []
    for ky in (0, 1):
        for kx in (0, 1):
            px, wt = tap_pixels(x, ky, kx), w[:, :, ky, kx]
            out.append((px @ wt.T, np.abs(px) @ np.abs(wt).T))
    return out


def space2depth(x, w, b, relu=False):
    """Conv2d(cin, cout, 2, stride=2): y[b, y, x, n] = sum_{ky, kx, c} x[b, 2y + ky, 2x + kx, c] w[n, c, ky, kx] + b[n]"""
    taps = space2depth_taps(x, w)
    return finish(sum(t[0] for t in taps), sum(t[1] for t in taps), b, relu=relu)


def depth2space_taps(x, w):
    """[(acc, S)] per tap ky * 2 + kx of ConvTranspose2d(k2, s2), each (B, H, W, cout): what the tap writes to pixels (2y + ky, 2x + kx)"""
    x, w = f64(x), f64(w)
    return [(x @ w[:, :, ky, kx], np.abs(x) @ np.abs(w[:, :, ky, kx])) for ky in (0, 1) for kx in (0, 1)]


def interleave_taps(planes):
    """four (B, H, W, C) planes in tap order -> the (B, 2H, 2W, C) map with plane ky * 2 + kx at pixels (2y + ky, 2x + kx)"""
    B, H, W, C = planes[0].shape
    out = np.empty((B, 2 * H, 2 * W, C), np.float64)
    for t, p in enumerate(planes):
        out[:, (t >> 1)::2, (t & 1)::2, :] = p
    return out


def depth2space(x, w, b, relu=False):
    """ConvTranspose2d(cin, cout, 2, stride=2): y[b, 2y + ky, 2x + kx, n] = sum_c x[b, y, x, c] w[c, n, ky, kx] + b[n]"""
    taps = depth2space_taps(x, w)
    return finish(interleave_taps([t[0] for t in taps]), interleave_taps([t[1] for t in taps]), b, relu=relu)


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------

def map_rows(rows, lattice):
    """pixel index of every row r < rows: r itself, or with lattice = (grid_h, grid_w, ky, kx) the pixel (b, 2y + ky, 2x + kx) of the
    (2 grid_h, 2 grid_w) map for r = (b, y, x) on the (grid_h, grid_w) grid"""
    r = np.arange(rows, dtype=np.int64)
    if lattice is None:
        return r
    gh, gw, ky, kx = lattice
    x, y, b = r % gw, (r // gw) % gh, r // (gw * gh)
    return (b * 2 * gh + 2 * y + ky) * 2 * gw + 2 * x + kx


def pw_wgrad(a, b, map_a, map_b, rows):
    """a (pixels_a, n), b (pixels_b, k): out[n, k] = sum_{r < rows} a[map_a(r), n] b[map_b(r), k] and the sum of |.||.| -> (out, S)"""
    ar = f64(a).reshape(-1, a.shape[-1])[map_rows(rows, map_a)]
    br = f64(b).reshape(-1, b.shape[-1])[map_rows(rows, map_b)]
    return ar.T @ br, np.abs(ar).T @ np.abs(br)


def pw_split(rows, n, k):
    """the split-K plan of pcp_pointwise_wgrad, restated from its description: 128 rows per chunk, the chunks dealt round-robin to
    nsplit = min(512 / pairs, 256, chunks) workgroups per 64x64 output tile: (chunks, nsplit)"""
    chunks = (rows + PW_ROWS - 1) // PW_ROWS
    pairs = ((n + 63) // 64) * ((k + 63) // 64)
    return chunks, max(1, min(512 // pairs, 256, chunks))


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every case names the code path it is there for
# ---------------------------------------------------------------------------------------------------------------------

Plain = namedtuple('Plain', 'rows cin cout relu res k_split why')        # res: None | 'after' | 'before';  k_split: 0 = single source
Spatial = namedtuple('Spatial', 'B H W cin cout relu why')
Wgrad = namedtuple('Wgrad', 'n k rows why')

PLAIN_CASES = [
    Plain(1, 16, 1, False, None, 0, 'one row, one slice, one channel: 128x32, scalar tail only, every other lane masked'),
    Plain(127, 48, 9, True, None, 0, 'one short row block; three slices (odd count: the prefetch ends on the other register set); tail of 1'),
    Plain(128, 16, 20, False, None, 0, 'exactly one row block; 128x32 with whole channel quads past cout masked'),
    Plain(129, 48, 32, True, None, 0, 'a second row block of ONE row; the full 32-channel tile'),
    Plain(300, 256, 70, True, None, 0, '128x64, two channel tiles, the second ending in a tail of 2; 16 slices; ragged rows'),
    Plain(1000, 256, 128, False, None, 0, '128x64 full tiles without activation; eight row blocks, the last ragged'),
    Plain(257, 48, 70, False, None, 0, '128x64 at an odd slice count; third row block of one row'),
    # two-source K (DiscoNet's weightor: cat([ego, other]) without the copy)
    Plain(200, 64, 20, True, None, 16, 'k_split after the FIRST slice: three slices from x2'),
    Plain(200, 64, 70, False, None, 48, 'k_split before the LAST slice (cin - 16); 128x64'),
    Plain(131, 64, 128, True, None, 32, 'k_split = cin / 2, the weightor\'s form'),
    # residual (heads with a skip, SCBottleneck's relu(conv3 + identity))
    Plain(150, 48, 9, True, 'after', 0, 'residual after the activation, cout % 4 == 1: reads masked at the tail'),
    Plain(150, 48, 9, True, 'before', 0, 'residual inside the activation (PCP_RELU_PRE_RESIDUAL), cout % 4 == 1'),
    Plain(129, 16, 70, True, 'after', 0, 'residual after, cout % 4 == 2, 128x64'),
    Plain(129, 16, 70, True, 'before', 0, 'residual inside, cout % 4 == 2, 128x64'),
    Plain(260, 256, 11, True, 'after', 0, 'residual after, cout % 4 == 3'),
    Plain(260, 256, 11, True, 'before', 0, 'residual inside, cout % 4 == 3'),
    Plain(140, 32, 67, False, 'after', 0, 'residual without any activation, cout % 4 == 3 in the second channel tile of 128x64'),
    Plain(133, 64, 30, True, 'before', 32, 'two sources AND a residual inside the activation (both PLAIN extras at once)'),
]

S2D_CASES = [
    Spatial(3, 6, 10, 16, 9, True, 'H != W, batch 3: 45 rows in one block; one slice per tap; 128x32 with a tail of 1'),
    Spatial(1, 4, 6, 48, 32, False, 'batch 1; three slices per tap (tap = slice / 3, channel = slice % 3)'),
    Spatial(1, 18, 30, 16, 70, True, '135 rows: a second, ragged row block whose rows start mid-row of the map; 128x64, tail of 2'),
    Spatial(3, 10, 12, 256, 128, False, 'K = 1024 in 64 slices; 128x64 full tiles'),
    Spatial(2, 12, 22, 48, 20, True, '132 rows over two blocks on 128x32, whole channel quads masked'),
    Spatial(1, 2, 2, 16, 1, False, 'a single output pixel and channel'),
]

D2S_CASES = [
    Spatial(3, 5, 7, 16, 9, True, 'H != W (odd both), batch 3: 105 rows; 128x32, one channel tile per tap; tail of 1'),
    Spatial(1, 3, 5, 48, 32, False, 'batch 1; odd slice count; full 32-channel tile per tap'),
    Spatial(1, 10, 13, 16, 70, True, '130 rows: second row block; 128x64 with cout_pad 128: tap = tile / 2; tail of 2'),
    Spatial(3, 6, 8, 256, 128, False, '16 slices; 128x64, eight full channel tiles'),
    Spatial(2, 9, 8, 48, 20, False, '144 rows over two blocks on 128x32, whole channel quads masked'),
    Spatial(1, 1, 1, 16, 1, False, 'one input pixel: four output pixels of one channel'),
]

# exact placement: 0/1 selection weights, small-integer inputs, bit-equal outputs
PLACE_PLAIN = Plain(131, 48, 70, False, None, 0, 'every output channel copies one input channel')
PLACE_S2D = Spatial(3, 6, 10, 16, 20, False, 'every output channel copies one (tap, channel) of its 2x2 block')
PLACE_D2S = Spatial(3, 5, 7, 48, 9, False, 'every tap has its own channel permutation')

WGRAD_CASES = [
    Wgrad(4, 4, 200, 'one quadrant of one tile: four waves share the chunk\'s rows and sum through LDS'),
    Wgrad(72, 40, 377, 'n and k no multiples of 64: n_r / k_r padding, a second n tile with 8 channels, two quadrants; ragged last chunk'),
    Wgrad(64, 64, 1, 'a single row'),
    Wgrad(64, 64, 127, 'one short chunk'),
    Wgrad(64, 64, 128, 'exactly one chunk'),
    Wgrad(64, 64, 129, 'a second chunk of one row'),
    Wgrad(128, 260, 300, 'ten tile pairs; the last k tile holds 4 channels'),
    Wgrad(256, 256, 1000, 'sixteen tile pairs, 8 chunks over 8 splits: one trip each'),
    Wgrad(256, 256, 8229, '65 chunks over 32 splits: one workgroup makes three trips of the chunk loop, the rest two (prefetch under the MFMAs, '
                           'LDS reuse behind the barrier); the last chunk has 37 rows'),
]

# lattice row maps: (n, k, batch, grid_h, grid_w) -- a non-square grid, batch 3, 105 rows
WGRAD_LATTICE = (72, 40, 3, 5, 7)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def plain_data(i):
    """inputs (float32) and the reference (y, S, K) of PLAIN_CASES[i], computed once and read-only"""
    c = PLAIN_CASES[i]
    x = uniform(100 + i, 1, (c.rows, c.cin))
    w = uniform(100 + i, 2, (c.cout, c.cin), -0.1, 0.1)
    b = uniform(100 + i, 3, (c.cout,), -0.2, 0.2)
    res = uniform(100 + i, 4, (c.rows, c.cout)) if c.res else None
    if c.k_split:
        y, S = plain(x[:, :c.k_split], w, b, x[:, c.k_split:], c.k_split, res, c.relu, c.res == 'before')
    else:
        y, S = plain(x, w, b, residual=res, relu=c.relu, residual_before_relu=c.res == 'before')
    return _frozen(dict(x=x, w=w, b=b, res=res, y=y, S=S, K=c.cin))


@functools.lru_cache(maxsize=None)
def spatial_data(kind, i):
    """the same for S2D_CASES[i] (kind 's2d') / D2S_CASES[i] (kind 'd2s'); x is NHWC"""
    c = (S2D_CASES if kind == 's2d' else D2S_CASES)[i]
    seed = (200 if kind == 's2d' else 300) + i
    x = uniform(seed, 1, (c.B, c.H, c.W, c.cin))
    b = uniform(seed, 3, (c.cout,), -0.2, 0.2)
    if kind == 's2d':
        w = uniform(seed, 2, (c.cout, c.cin, 2, 2), -0.1, 0.1)
        y, S = space2depth(x, w, b, c.relu)
        K = 4 * c.cin
    else:
        w = uniform(seed, 2, (c.cin, c.cout, 2, 2), -0.1, 0.1)
        y, S = depth2space(x, w, b, c.relu)
        K = c.cin
    return _frozen(dict(x=x, w=w, b=b, y=y, S=S, K=K))


@functools.lru_cache(maxsize=None)
def wgrad_data(i):
    c = WGRAD_CASES[i]
    a = uniform(400 + i, 1, (c.rows, c.n))
    b = uniform(400 + i, 2, (c.rows, c.k))
    out, S = pw_wgrad(a, b, None, None, c.rows)
    return _frozen(dict(a=a, b=b, out=out, S=S, K=c.rows))


def selection_plain(seed, cout, cin):
    """w (cout, cin) with one 1 per row at a seeded input channel, and that channel list"""
    pick = np.argsort(uniform(seed, 9, (max(cout, cin),)))[:cout] % cin
    w = np.zeros((cout, cin), np.float32)
    w[np.arange(cout), pick] = 1.0
    return w, pick
