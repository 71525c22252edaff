"""Plain float64 references (numpy, no GPU) of the forward kernels of the bf16 training loop, their weight packs, and the case tables
their tests share.

  conv3x3, conv3x3_dgrad     pcp_mp_conv3x3: k_mp_conv3x3_s1 (stride 1, bf16 in, cin % 32 == 0) and k_mp_conv3x3_gen   (csrc/mp_conv.hip)
  pack_expect, unpack3x3     pcp_mp_pack_conv3x3 / pcp_mp_pack_conv3x3_group: k_mp_pack3x3, k_mp_pack3x3_group          (csrc/mp_conv.hip)
  pw_pack + the references   pcp_mp_pointwise (k_mp_pw, three modes) and pcp_mp_pointwise_wgrad (k_mp_pw_wgrad)          (csrc/mp_pointwise.hip)
  of pointwise_refs.py

Maps are NHWC; 3x3 weights have torch's layout (cout, cin, 3, 3); float32 inputs enter the arithmetic as their exact float64 values.

Three kinds of input, as in tests/wgrad3x3_refs.py.  Integers: maps and weights hold non-zero integers in [-8, 8], the bias integers in
[-8, 8]; every product and every partial sum is an integer below 2^24 (tests/test_mp_forward_refs_cpu.py asserts max S < 2^22 for every
case), exact in fp32 in ANY order and exact as bf16 operands, so the kernels owe the float64 result bit for bit, and a bf16 output owes
its round-to-nearest-even: integers above 256 are no bf16 values, and the odd ones between 256 and 512 are exact ties.  Ties: fp32 maps
of k + 0.5, k in [128, 255], exact ties of the fp32 -> bf16 rounding whose two outcomes are integers.  Floats: uniform maps and weights
rounded to bf16; the tolerance is 2 * bound(S, K) element by element, the rule wgrad3x3_refs.py states for the bf16 matrix unit (exact
products, adds that may truncate), with S the sum of |x||w| plus |b| and K the number of products plus one for the bias.
"""
import functools
from collections import namedtuple

import numpy as np

from pointwise_refs import (WGRAD_CASES, WGRAD_LATTICE, bound, depth2space, f64, map_rows, plain, pw_wgrad,  # noqa: F401  (the tests reach
                            selection_plain, small_ints, space2depth, uniform)                               # them through this module)
from wgrad3x3_refs import bf16_round, tap_view

INT_MAX = 8                      # integer variants hold integers in [-8, 8]
MC_TW, MC_CK, MC_BN = 32, 32, 64 # k_mp_conv3x3_s1: pixels per item row, channels per stage, output channels per item
MC_MAX_COUT = 512                # widest bias row of the fast kernel
MG_TW = 16                       # k_mp_conv3x3_gen: 16x16 (stride 1) / 8x16 (stride 2) output pixels per workgroup
MPW_BM = 128                     # k_mp_pw: pixels per workgroup
MWG_ROWS, MWG_NST = 32, 4        # k_mp_pw_wgrad: rows per stage, stages resident
CUS = 256                        # compute units of the MI355X: the fast kernel launches min(items, CUs) persistent workgroups


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 references
# ---------------------------------------------------------------------------------------------------------------------

def _padded(x):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), np.float64)
    xp[:, 1:H + 1, 1:W + 1, :] = x
    return xp


def conv3x3(x, w, b, stride, relu):
    """y[b, oy, ox, n] = sum_{ky, kx, c} x[b, oy s + ky - 1, ox s + kx - 1, c] w[n, c, ky, kx] + b[n] (x = 0 outside the map; output
    (H - 1) // s + 1 by (W - 1) // s + 1, odd H and W at stride 2 included) and S = the same sum of |x||w| plus |b|: (y, S), nine
    shifted-slice matmuls.  relu clamps y; S stays the bound's scale (relu is 1-Lipschitz)"""
    x, w, b = f64(x), f64(w), f64(b)
    B, H, W, cin = x.shape
    cout = w.shape[0]
    assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,)
    Ho, Wo = out_hw(H, W, stride)
    xp = _padded(x)
    y = np.zeros((B * Ho * Wo, cout), np.float64)
    S = np.zeros((B * Ho * Wo, cout), np.float64)
    for ky in range(3):
        for kx in range(3):
            t = np.ascontiguousarray(tap_view(xp, ky, kx, Ho, Wo, stride)).reshape(-1, cin)
            y += t @ w[:, :, ky, kx].T
            S += np.abs(t) @ np.abs(w[:, :, ky, kx]).T
    y, S = y + b, S + np.abs(b)
    if relu:
        y = np.maximum(y, 0.0)
    return y.reshape(B, Ho, Wo, cout), S.reshape(B, Ho, Wo, cout)


def conv3x3_dgrad(dy, w):
    """the stride-1 data gradient dx[b, y, x, ci] = sum_{co, ky, kx} dy[b, y - (ky - 1), x - (kx - 1), co] w[co, ci, ky, kx], written as
    the scatter it is: every dy pixel adds dy w[:, :, ky, kx] to its neighbour at (+ ky - 1, + kx - 1); what leaves the map is dropped.
    (dx, S); no weight is flipped or transposed here"""
    dy, w = f64(dy), f64(w)
    B, H, W, cout = dy.shape
    cin = w.shape[1]
    assert w.shape == (cout, cin, 3, 3)
    dxp = np.zeros((B, H + 2, W + 2, cin), np.float64)
    Sp = np.zeros((B, H + 2, W + 2, cin), np.float64)
    d2 = dy.reshape(-1, cout)
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + H, kx:kx + W, :] += (d2 @ w[:, :, ky, kx]).reshape(B, H, W, cin)
            Sp[:, ky:ky + H, kx:kx + W, :] += (np.abs(d2) @ np.abs(w[:, :, ky, kx])).reshape(B, H, W, cin)
    return dxp[:, 1:H + 1, 1:W + 1, :].copy(), Sp[:, 1:H + 1, 1:W + 1, :].copy()


def taps_inside(H, W, stride):
    """(Ho, Wo): how many of the nine taps of an output pixel lie inside the map (the others multiply exact zeros)"""
    Ho, Wo = out_hw(H, W, stride)
    ny = sum(((np.arange(Ho) * stride + k - 1 >= 0) & (np.arange(Ho) * stride + k - 1 < H)).astype(np.int64) for k in range(3))
    nx = sum(((np.arange(Wo) * stride + k - 1 >= 0) & (np.arange(Wo) * stride + k - 1 < W)).astype(np.int64) for k in range(3))
    return ny[:, None] * nx[None, :]


# ---------------------------------------------------------------------------------------------------------------------
# weight packs
# ---------------------------------------------------------------------------------------------------------------------

def pack_expect(w, fold, transpose):
    """the bf16 values k_mp_pack3x3 owes, as float32 that hold bf16 values, in logical (out, contraction, ky, kx) order where (ky, kx) is
    the tap the KERNEL applies the value at.  The packer's arithmetic: the fp32 product w * fold[co] (co = the weight tensor's first
    axis in either form; 1 without fold_scale), then ONE rounding to the nearest bf16, ties to even.
      forward    (out, contraction) = (cout, cin):  v[o, k, ky, kx] = w[o, k, ky, kx] * fold[o]
      transpose  (out, contraction) = (cin, cout):  v[o, k, ky, kx] = w[k, o, 2 - ky, 2 - kx] * fold[k]      (tap 8 - t)"""
    w = np.asarray(w, np.float32)
    f = np.ones(w.shape[0], np.float32) if fold is None else np.asarray(fold, np.float32)
    v = w * f[:, None, None, None]                                   # float32 x float32 -> float32, rounded once as the device's multiply
    assert v.dtype == np.float32
    if transpose:
        v = v.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    return bf16_round(np.ascontiguousarray(v))


def unpack3x3(packed, contraction, out_pad):
    """the packed layout [contraction / 16][out_pad / 64][9 (ky * 3 + kx)][2 (k half)][64 (out)][8 (k)] of include/pcp_hip_mp.h, flat,
    any dtype -> (out_pad, contraction, 3, 3): out = block * 64 + o64, k = slice * 16 + half * 8 + j"""
    a = np.asarray(packed).reshape(contraction // 16, out_pad // 64, 9, 2, 64, 8)
    return np.ascontiguousarray(a.transpose(1, 4, 0, 3, 5, 2)).reshape(out_pad, contraction, 3, 3)


def bf16_bits(a):
    """float32 that hold bf16 values -> their 16 bits"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def pw_pack(kind, w, b, cout_pad):
    """the pointwise weight form [k_total / 16][n_total][16] (float32 here, cast to bf16 by the caller) and the padded bias:
      plain  w (cout, cin)         k = c,                        n = co                          n_total = cout_pad
      s2d    w (cout, cin, 2, 2)   k = (ky * 2 + kx) * cin + c,  n = co                          n_total = cout_pad
      d2s    w (cin, cout, 2, 2)   k = c,                        n = (ky * 2 + kx) * cout_pad + co   n_total = 4 * cout_pad
    cout_pad is the caller's (pcp_mp_pointwise wants a multiple of 64, also below 32 channels)"""
    w = np.asarray(w, np.float32)
    if kind == 'plain':
        cout = w.shape[0]
        mat = np.zeros((cout_pad, w.shape[1]), np.float32)
        mat[:cout] = w.reshape(cout, -1)
    elif kind == 's2d':
        cout, cin = w.shape[:2]
        mat = np.zeros((cout_pad, 4 * cin), np.float32)
        mat[:cout] = w.transpose(0, 2, 3, 1).reshape(cout, 4 * cin)
    else:
        cin, cout = w.shape[:2]
        mat = np.zeros((4, cout_pad, cin), np.float32)
        mat[:, :cout] = w.transpose(2, 3, 1, 0).reshape(4, cout, cin)
        mat = mat.reshape(4 * cout_pad, cin)
    n, k = mat.shape
    bp = np.zeros(cout_pad, np.float32)
    bp[:len(b)] = b
    return np.ascontiguousarray(mat.reshape(n, k // 16, 16).transpose(1, 0, 2)), bp


# ---------------------------------------------------------------------------------------------------------------------
# input generators
# ---------------------------------------------------------------------------------------------------------------------

def ints8(seed, col, shape):
    """non-zero integers in [-8, 8], float32"""
    return np.clip(small_ints(seed, col, shape), -INT_MAX, INT_MAX).astype(np.float32)


def tie_ints(seed, col, shape):
    """+-(k + 0.5), k in [128, 255]: exact in fp32, exact ties in bf16 (spacing 1 there); nearest-even gives the even neighbour,
    truncation gives k, rounding half away gives k + 1 -- all integers"""
    k = np.clip(np.floor(f64(uniform(seed, col, shape, 128.0, 256.0))), 128, 255)
    sign = np.where(uniform(seed, col + 1, shape) < 0, -1.0, 1.0)
    return ((k + 0.5) * sign).astype(np.float32)


def tie_weights(seed, col, shape):
    """+-(1 + (2 m + 1) 2^-8) 2^e, m in [0, 63], e in [-4, 0]: exact in fp32, exact ties on the bf16 grid of [1, 2) (spacing 2^-7)
    scaled by a power of two"""
    m = np.clip(np.floor(f64(uniform(seed, col, shape, 0.0, 64.0))), 0, 63)
    e = np.clip(np.floor(f64(uniform(seed, col + 1, shape, -4.0, 1.0))), -4, 0)
    sign = np.where(uniform(seed, col + 2, shape) < 0, -1.0, 1.0)
    return (sign * (1.0 + (2.0 * m + 1.0) * 2.0 ** -8) * 2.0 ** e).astype(np.float32)


def tie_fold(seed, col, n):
    """fold_scale for tie weights: even entries powers of two (the products stay exact ties), odd entries arbitrary (the fp32 product is
    rounded before the bf16 rounding, and a fold applied to bf16-rounded weights lands elsewhere)"""
    f = uniform(seed, col, (n,), 0.5, 1.5)
    p = 2.0 ** np.clip(np.floor(f64(uniform(seed, col + 1, (n,), -2.0, 2.0))), -2, 1)
    return np.where(np.arange(n) % 2 == 0, p, f).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every case names the code path it is there for
# ---------------------------------------------------------------------------------------------------------------------

# ins / outs: the storage types the case runs in ('bf16', 'f32'); th: 0 = the library's item-size rule (8 rows for every such case), 16 / 8 =
# run under lib_option('mp_th16_min', 1 / TH8_MIN), which makes the rule choose 16-row / 8-row items
Conv = namedtuple('Conv', 'cin cout B H W stride relu ins outs th why')
TH8_MIN = 1 << 20
BOTH, BF, F32 = ('bf16', 'f32'), ('bf16',), ('f32',)

FAST_CASES = [
    Conv(32, 64, 1, 8, 32, 1, True, BF, BOTH, 0, 'one item of one stage'),
    Conv(64, 64, 1, 9, 33, 1, False, BF, BOTH, 0, 'one row and one column past a tile: the last tiles are 1 wide and 1 high'),
    Conv(96, 72, 2, 7, 31, 1, True, BF, BOTH, 0, 'odd slice count, masked channel groups; bf16 out needs cout % 8'),
    Conv(64, 132, 1, 16, 40, 1, False, BF, F32, 0, 'cout % 4 (fp32 out only), three channel blocks'),
    Conv(384, 64, 1, 8, 32, 1, True, BF, BOTH, 0, '12 slices'),
    Conv(64, 512, 1, 8, 32, 1, False, BF, BOTH, 0, 'MC_MAX_COUT: the whole bias row in LDS, eight channel blocks'),
    Conv(64, 64, 3, 17, 70, 1, True, BF, BOTH, 0, 'three frames of 3x3 ragged tiles (17 = 2 x 8 + 1, 70 = 2 x 32 + 6): 27 items, one per workgroup'),
    Conv(64, 64, 1, 17, 33, 1, True, BF, BOTH, 16, '16-row items: a second tile row and column of one pixel'),
    Conv(64, 128, 2, 33, 31, 1, False, BF, BOTH, 16, '16-row items: three tile rows, two frames, two channel blocks'),
    Conv(128, 64, 1, 16, 32, 1, True, BF, BOTH, 16, '16-row items: exactly one item, four slices'),
    Conv(32, 256, 6, 48, 64, 1, False, BF, BOTH, 0, '288 eight-row items on 256 workgroups with ONE slice each: 32 workgroups copy stage 0 of '
                                                   'a second item under the products of the first -- the next channel block of the SAME tile'),
    Conv(64, 320, 26, 9, 33, 1, True, BF, BOTH, 8, '520 eight-row items (2x2 tiles x 5 channel blocks x 26 frames) of two slices: the first eight '
                                                   'workgroups walk three items each and step to the next tile column, tile row and frame inside a run'),
    Conv(64, 320, 26, 17, 33, 1, False, BF, BOTH, 16, 'the same runs of 16-row items (eight waves): tile column, tile row and frame steps inside a run'),
]

GEN_CASES = [
    Conv(16, 64, 1, 1, 1, 1, False, BOTH, BOTH, 0, 'one pixel: only the centre tap is inside the map'),
    Conv(16, 64, 1, 19, 23, 1, True, F32, F32, 0, 'fp32 in, fp32 out; 2x2 tiles of 16x16, ragged both ways'),
    Conv(48, 64, 1, 17, 17, 1, False, BF, BOTH, 0, 'bf16 in with cin % 32 == 16; second tile row and column of one pixel'),
    Conv(64, 64, 2, 16, 32, 2, True, BOTH, BOTH, 0, 'stride 2, even map: the last pixel\'s bottom and right taps are inside the map'),
    Conv(64, 128, 2, 15, 33, 2, False, BOTH, BOTH, 0, 'stride 2, odd H and W: the last row and column read their halo outside the map'),
    Conv(32, 40, 2, 9, 9, 1, True, F32, BF, 0, 'fp32 in, bf16 out at stride 1; masked output channels'),
    Conv(32, 40, 2, 9, 9, 2, False, F32, BF, 0, 'the same at stride 2: output 5x5 of an odd map'),
]

CONV_TABLES = {'fast': FAST_CASES, 'gen': GEN_CASES}

# the bf16 window that starts 8 but not 16 bytes into a pixel record: the general kernel, although mc_fast_ok holds
MISALIGNED = Conv(64, 64, 1, 8, 32, 1, True, BF, BOTH, 0, 'in_ch_off 4 of ld_in 72: an 8-byte aligned bf16 window')

# channel windows: (table, index) x both output types; the offsets keep 16-byte alignment
WINDOW_CASES = [('fast', 1), ('fast', 2), ('gen', 2), ('gen', 4)]

# one-hot placement: (table, index, data-gradient form)
PLACE_CASES = [('fast', 1, False), ('fast', 1, True), ('fast', 7, False), ('fast', 11, False), ('fast', 12, True), ('gen', 2, False),
               ('gen', 2, True), ('gen', 4, False)]

Pw = namedtuple('Pw', 'kind B H W cin cout relu why')                    # plain: B = rows, H = W = 0

PW_CASES = [
    Pw('plain', 1, 0, 0, 32, 8, False, 'one row, one slice, one channel group; 63 masked channels'),
    Pw('plain', 127, 0, 0, 96, 72, True, 'one short pixel block; odd slice count; a second channel tile with 8 channels'),
    Pw('plain', 128, 0, 0, 32, 64, False, 'exactly one pixel block and one channel tile'),
    Pw('plain', 129, 0, 0, 512, 8, True, 'a second pixel block of ONE row; 16 slices'),
    Pw('plain', 385, 0, 0, 96, 64, True, 'a fourth pixel block of one row'),
    Pw('s2d', 1, 2, 2, 32, 8, False, 'a single output pixel'),
    Pw('s2d', 2, 6, 10, 96, 72, True, 'batch 2, H != W: 30 rows; three slices per tap'),
    Pw('s2d', 1, 16, 18, 32, 64, False, '72 rows of a 9-wide output'),
    Pw('s2d', 2, 16, 18, 32, 64, True, '144 rows: the second 128-pixel block starts mid-row of the second frame'),
    Pw('d2s', 1, 1, 1, 32, 8, False, 'one input pixel: four output pixels'),
    Pw('d2s', 3, 5, 7, 96, 72, True, 'batch 3, odd H and W: 105 rows; cout_pad 128, tap = tile / 2'),
    Pw('d2s', 1, 8, 17, 512, 64, False, '136 rows: a second pixel block; 16 slices'),
]

# the shapes of pointwise_refs.WGRAD_CASES with channels % 8 == 0 and one more; the reasons are those of k_mp_pw_wgrad (32-row stages, pwg_split)
Wgrad = namedtuple('Wgrad', 'n k rows why')
_PWG_WHY = {
    (72, 40, 377): 'n and k no multiples of 64: a second n tile with 8 channels, masked 16-byte pieces; 12 stages in one split, the last of 25 rows',
    (64, 64, 1): 'a single row',
    (64, 64, 127): 'four stages, the last one row short: the ring is exactly full',
    (64, 64, 128): 'exactly four stages',
    (64, 64, 129): 'a fifth stage of one row: the ring of four wraps',
    (256, 256, 1000): 'sixteen tiles; 32 stages over 4 splits of eight',
    (256, 256, 8229): '258 stages over 32 splits: two workgroups walk nine, the rest eight; the last stage holds 5 rows',
}
PWG_CASES = [Wgrad(c.n, c.k, c.rows, _PWG_WHY[(c.n, c.k, c.rows)]) for c in WGRAD_CASES if c.n % 8 == 0 and c.k % 8 == 0] + [
    Wgrad(64, 64, 161, 'rows = 32 * 5 + 1: one workgroup walks six stages, the ring of four wraps, the last stage holds one row'),
]


def pwg_split(rows, n, k):
    """the split plan of pcp_mp_pointwise_wgrad, restated from mwg_split: 32-row stages dealt round-robin to about 1024 / tiles workgroups
    per 64x64 tile, at least eight stages each, at most 512: (stages, nsplit)"""
    chunks = -(-rows // MWG_ROWS)
    tiles = (-(-n // 64)) * (-(-k // 64))
    return chunks, max(1, min(-(-1024 // tiles), chunks // 8, 512))


def conv_items(c, th):
    """work items of k_mp_conv3x3_s1 at th-row items"""
    return c.B * (-(-c.H // th)) * (-(-c.W // MC_TW)) * (-(-c.cout // MC_BN))


def fast_runs(c, th, cus=CUS):
    """the contiguous run of items [begin, end) of every workgroup of k_mp_conv3x3_s1, restated from its description: min(items, CUs)
    workgroups; workgroup l walks per + (l < rem) items from l * per + min(l, rem), per = items // workgroups, rem = items % workgroups"""
    n = conv_items(c, th)
    nwg = min(n, cus)
    per, rem = n // nwg, n % nwg
    return [(l * per + min(l, rem), l * per + min(l, rem) + per + (1 if l < rem else 0)) for l in range(nwg)]


def item_coords(c, th, it):
    """item -> (frame, tile row, tile column, channel block): the 64-channel block runs fastest, then the tile column, the tile row, the frame"""
    n_nb, tiles_x, tiles_y = -(-c.cout // MC_BN), -(-c.W // MC_TW), -(-c.H // th)
    nb, sp = it % n_nb, it // n_nb
    return sp // (tiles_x * tiles_y), (sp // tiles_x) % tiles_y, sp % tiles_x, nb


def run_steps(c, th):
    """what changes between consecutive items INSIDE the runs of fast_runs: the set of 'nb' (next channel block of the same tile), 'tx' (next
    tile column), 'ty' (the column wraps, next tile row), 'frame' (column and row wrap, next frame)"""
    kinds = set()
    for begin, end in fast_runs(c, th):
        for it in range(begin, end - 1):
            (b0, y0, x0, _n0), (b1, y1, x1, _n1) = item_coords(c, th, it), item_coords(c, th, it + 1)
            kinds.add('frame' if b1 != b0 else 'ty' if y1 != y0 else 'tx' if x1 != x0 else 'nb')
    return kinds


def tile_rows(c, min16=256):
    """mc_tile_rows, restated: 16-row items once they number min16, else 8-row items"""
    return 16 if conv_items(c, 16) >= min16 else 8


def fast_plan(c):
    """pcp_mp_conv3x3_plan's kernel choice, restated from mc_fast_ok, for bf16 input at a 16-byte aligned pointer"""
    return c.stride == 1 and c.cin % MC_CK == 0 and -(-c.cout // 64) * 64 <= MC_MAX_COUT


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def tie_bias(acc, b, relu):
    """choose the bias of up to two output channels so that one element of each becomes an odd integer in (256, 512) in magnitude: an
    exact tie of the bf16 store, reached only when the bias is added BEFORE the rounding.  One positive and, without a ReLU, one negative.
    Returns [(flat pixel, channel)] of the ties made; b is changed in place, inside [-2, 2]"""
    flat = acc.reshape(-1, acc.shape[-1])
    made = []
    for sign in ((1, 1) if relu else (1, -1)):
        for n in range(flat.shape[1]):
            if any(n == m for _p, m in made):
                continue
            v = flat[:, n] * sign
            hit = np.nonzero((v >= 260) & (v <= 500))[0]
            if len(hit):
                p = int(hit[0])
                b[n] = sign * (1.0 if flat[p, n] % 2 == 0 else 2.0)
                made.append((p, n))
                break
    return made


@functools.lru_cache(maxsize=None)
def conv_data(table, i, variant, dgrad=False):
    """inputs (float32) and the reference of CONV_TABLES[table][i] (or MISALIGNED for table 'mis'), computed once and read-only.
    variant 'ints' | 'float' | 'ties' (fp32 maps of tie_ints: the reference is taken on bf16_round(x)).  dgrad: the data-gradient form --
    the kernel's cin input channels are dy's, w is the (cin, cout, 3, 3) tensor of the conv whose gradient it is, no bias, no ReLU.
    y is the result, pre the value before the ReLU; K is per element: products inside the map plus one"""
    c = MISALIGNED if table == 'mis' else CONV_TABLES[table][i]
    seed = {'fast': 1000, 'gen': 2000, 'mis': 2900}[table] + 20 * i + {'ints': 0, 'float': 5, 'ties': 10}[variant] + (3 if dgrad else 0)
    shape_x = (c.B, c.H, c.W, c.cin)
    shape_w = (c.cin, c.cout, 3, 3) if dgrad else (c.cout, c.cin, 3, 3)
    ties = []
    if variant == 'float':
        x, w = bf16_round(uniform(seed, 1, shape_x)), bf16_round(uniform(seed, 2, shape_w, -0.2, 0.2))
        b = uniform(seed, 3, (c.cout,), -0.5, 0.5)
    else:
        x = ints8(seed, 1, shape_x) if variant == 'ints' else tie_ints(seed, 1, shape_x)
        w = ints8(seed, 3, shape_w)
        b = np.round(uniform(seed, 5, (c.cout,), -8.0, 8.0)).astype(np.float32)
    xr = bf16_round(x)
    if dgrad:
        assert c.stride == 1
        b = np.zeros(c.cout, np.float32)
        pre, S = conv3x3_dgrad(xr, w)
        relu = False
    else:
        relu = c.relu
        acc, S = conv3x3(xr, w, np.zeros(c.cout), c.stride, False)
        if variant == 'ints':
            ties = tie_bias(acc, b, relu)
        pre, S = acc + f64(b), S + np.abs(f64(b))                          # the bias is one more term, as in conv3x3
    y = np.maximum(pre, 0.0) if relu else pre
    K = taps_inside(c.H, c.W, c.stride)[None, :, :, None] * c.cin + 1
    return _frozen(dict(x=x, w=w, b=b, y=y, pre=pre, S=S, K=K, relu=relu, ties=ties))


def pw_out_shape(c):
    if c.kind == 'plain':
        return (c.B, c.cout)
    return (c.B, c.H // 2, c.W // 2, c.cout) if c.kind == 's2d' else (c.B, 2 * c.H, 2 * c.W, c.cout)


@functools.lru_cache(maxsize=None)
def pw_data(i, variant):
    """the same for PW_CASES[i]; weights in torch's layout of the kind"""
    c = PW_CASES[i]
    seed = 3000 + 20 * i + {'ints': 0, 'float': 5, 'ties': 10}[variant]
    shape_x = (c.B, c.cin) if c.kind == 'plain' else (c.B, c.H, c.W, c.cin)
    shape_w = {'plain': (c.cout, c.cin), 's2d': (c.cout, c.cin, 2, 2), 'd2s': (c.cin, c.cout, 2, 2)}[c.kind]
    if variant == 'float':
        x, w = bf16_round(uniform(seed, 1, shape_x)), bf16_round(uniform(seed, 2, shape_w, -0.2, 0.2))
        b = uniform(seed, 3, (c.cout,), -0.5, 0.5)
    else:
        x = ints8(seed, 1, shape_x) if variant == 'ints' else tie_ints(seed, 1, shape_x)
        w = ints8(seed, 3, shape_w)
        b = np.round(uniform(seed, 5, (c.cout,), -8.0, 8.0)).astype(np.float32)
    ref = {'plain': plain, 's2d': space2depth, 'd2s': depth2space}[c.kind]
    ties = []
    if variant == 'ints':
        acc, _S = ref(bf16_round(x), w, np.zeros(c.cout), relu=False)
        ties = tie_bias(acc, b, c.relu)
    pre, S = ref(bf16_round(x), w, b, relu=False)
    y = np.maximum(pre, 0.0) if c.relu else pre
    K = (4 * c.cin if c.kind == 's2d' else c.cin) + 1
    return _frozen(dict(x=x, w=w, b=b, y=y, pre=pre, S=S, K=K, relu=c.relu, ties=ties))


@functools.lru_cache(maxsize=None)
def pwg_data(i, ints):
    c = PWG_CASES[i]
    if ints:
        a, b = ints8(4000 + 10 * i, 1, (c.rows, c.n)), ints8(4000 + 10 * i, 3, (c.rows, c.k))
    else:
        a, b = bf16_round(uniform(4005 + 10 * i, 1, (c.rows, c.n))), bf16_round(uniform(4005 + 10 * i, 2, (c.rows, c.k)))
    out, S = pw_wgrad(a, b, None, None, c.rows)
    return _frozen(dict(a=a, b=b, out=out, S=S, K=c.rows))


def pwg_old(i):
    """the integer contents accumulate=1 adds the sums of PWG_CASES[i] onto: +-100 .. +-800"""
    c = PWG_CASES[i]
    return (100.0 * ints8(4900 + i, 1, (c.n, c.k))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice_data(side):
    """integer operands for the lattice row maps of WGRAD_LATTICE: the lattice on operand `side` ('a' | 'b', a (B, 2 gh, 2 gw, C) map), the
    identity on the other, and [(lattice, out, S)] for the four taps"""
    n, k, B, gh, gw = WGRAD_LATTICE
    rows = B * gh * gw
    big_c, small_c = (n, k) if side == 'a' else (k, n)
    big, small = ints8(4950, 1, (B, 2 * gh, 2 * gw, big_c)), ints8(4950, 3, (rows, small_c))
    taps = []
    for tap in range(4):
        lat = (gh, gw, tap >> 1, tap & 1)
        out, S = pw_wgrad(big, small, lat, None, rows) if side == 'a' else pw_wgrad(small, big, None, lat, rows)
        taps.append((lat, out, S))
    return _frozen(dict(big=big, small=small, rows=rows, taps=taps))


# ---------------------------------------------------------------------------------------------------------------------
# one-hot placement
# ---------------------------------------------------------------------------------------------------------------------

def one_hot_conv(seed, cin, cout, dgrad=False):
    """3x3 weights with a single 1.0 per KERNEL output channel n, at tap n % 9 (every tap is somebody's) and a seeded contraction channel:
    (w, [(ky, kx, c)] by n).  Forward: w (cout, cin, 3, 3), w[n, c, ky, kx] = 1.  dgrad: w (cin, cout, 3, 3), w[c, n, ky, kx] = 1"""
    pick = np.argsort(uniform(seed, 9, (max(cout, cin),)))[:cout] % cin
    w = np.zeros((cin, cout, 3, 3) if dgrad else (cout, cin, 3, 3), np.float32)
    picks = []
    for n in range(cout):
        ky, kx, ch = (n % 9) // 3, (n % 9) % 3, int(pick[n])
        if dgrad:
            w[ch, n, ky, kx] = 1.0
        else:
            w[n, ch, ky, kx] = 1.0
        picks.append((ky, kx, ch))
    return w, picks


def one_hot_conv_expect(x, picks, stride, dgrad=False):
    """what the one-hot weights make of the map x: output channel n is channel c of the pixel at (oy s + ky - 1, ox s + kx - 1) -- for
    the data gradient the OPPOSITE shift, (y - (ky - 1), x - (kx - 1)) -- and exactly 0 where that pixel is outside the map"""
    B, H, W, _cin = x.shape
    Ho, Wo = out_hw(H, W, stride)
    xp = _padded(f64(x))
    out = np.empty((B, Ho, Wo, len(picks)), np.float64)
    for n, (ky, kx, ch) in enumerate(picks):
        if dgrad:
            ky, kx = 2 - ky, 2 - kx
        out[..., n] = tap_view(xp, ky, kx, Ho, Wo, stride)[..., ch]
    return out


def place_map(seed, shape):
    """arbitrary non-zero values exact in bf16, read-only"""
    x = uniform(seed, 1, shape, 0.5, 2.0) * np.where(uniform(seed, 2, shape) < 0, np.float32(-1), np.float32(1))
    x = bf16_round(x)
    x.setflags(write=False)
    return x
