"""Plain float64 reference (numpy, no GPU) of the 3x3 weight gradient (stride 1 / 2, padding 1), the split plans of the two kernels that
compute it, restated from their descriptions, and the case tables their tests share.

  fp32   pcp_conv3x3_wgrad      k_wgrad3x3 + k_wgrad3x3_reduce       (csrc/wgrad.hip)
  bf16   pcp_mp_conv3x3_wgrad   k_mp_wgrad3x3 + k_mp_wgrad_reduce    (csrc/mp_wgrad.hip)

Maps are NHWC: x (B, H, W, cin), dy (B, H / s, W / s, cout); dw has torch's layout (cout, cin, 3, 3).  Float32 inputs enter the arithmetic
as their exact float64 values.

Two tolerances, both from tests/pointwise_refs.py.  Float inputs: bound(S, K), element by element, with S = sum |dy| |x| over the pixels
of the sum and K = B * Ho * Wo their number (the split partial sums and their reduction are additions of the same sum).  The bf16 kernel
multiplies bf16 operands exactly in fp32 (8 + 8 significand bits) and only its additions round; the matrix unit may truncate where an fp32
add rounds to nearest, one ulp per add instead of half: its tolerance is 2 * bound(S, K) on the bf16-rounded operands.  Integer inputs:
with x and dy small non-zero integers every product and every partial sum is an integer below 2^24, exact in fp32 in ANY order and
exact in bf16 storage, so both kernels owe the float64 result bit for bit (tests/test_wgrad3x3_refs_cpu.py asserts max S < 2^22 for every
case).
"""
import functools
from collections import namedtuple

import numpy as np

from pointwise_refs import bound, f64, small_ints, uniform  # noqa: F401  (bound is what the tests of these tables compare against)

INT_MAX = 8                      # integer variants hold non-zero integers in [-8, 8]
WG_DW = 32                       # dy columns of a strip of k_mp_wgrad3x3


def out_hw(H, W, stride):
    return H // stride, W // stride


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------

def tap_view(xp, ky, kx, Ho, Wo, stride):
    """of the zero-padded map xp (B, H + 2, W + 2, C): the pixels (oy * s + ky - 1, ox * s + kx - 1) of the unpadded one, (B, Ho, Wo, C)"""
    return xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]


def wgrad3x3(x, dy, stride):
    """dw[co, ci, ky, kx] = sum_{b, oy, ox} dy[b, oy, ox, co] x[b, oy s + ky - 1, ox s + kx - 1, ci] (x = 0 outside the map) and the same
    sum of |dy| |x|: (dw, S), float64, nine shifted-slice matmuls"""
    x, dy = f64(x), f64(dy)
    B, H, W, cin = x.shape
    Ho, Wo = out_hw(H, W, stride)
    cout = dy.shape[3]
    assert dy.shape == (B, Ho, Wo, cout) and (stride == 1 or (H % 2 == 0 and W % 2 == 0))
    xp = np.zeros((B, H + 2, W + 2, cin), np.float64)
    xp[:, 1:H + 1, 1:W + 1, :] = x
    d2 = dy.reshape(-1, cout)
    dw = np.empty((cout, cin, 3, 3), np.float64)
    S = np.empty((cout, cin, 3, 3), np.float64)
    for ky in range(3):
        for kx in range(3):
            t = np.ascontiguousarray(tap_view(xp, ky, kx, Ho, Wo, stride)).reshape(-1, cin)
            dw[:, :, ky, kx] = d2.T @ t
            S[:, :, ky, kx] = np.abs(d2).T @ np.abs(t)
    return dw, S


def one_hot_expect(x, b, oy, ox, stride):
    """what dw[co] is when dy holds a single 1.0, at (b, oy, ox, co): the 3x3 patch of x around (oy s, ox s), (cin, 3, 3), exactly 0 where
    the patch leaves the map"""
    _B, H, W, cin = x.shape
    out = np.zeros((cin, 3, 3), np.float64)
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
            if 0 <= iy < H and 0 <= ix < W:
                out[:, ky, kx] = f64(x[b, iy, ix, :])
    return out


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32; finite inputs"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# split plans, restated from the descriptions of plan3 (csrc/wgrad.hip) and wg_plan (csrc/mp_wgrad.hip)
# ---------------------------------------------------------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def tile_fp32(stride):
    """output pixels (rows, columns) of a pixel tile of k_wgrad3x3"""
    return (8, 16) if stride == 1 else (4, 8)


def plan_fp32(B, H, W, cin, cout, stride):
    """pixel tiles of 8x16 (stride 1) or 4x8 (stride 2) output pixels, dealt round-robin to nsplit = min(256 / pairs, n_tiles) workgroups
    per 64x64 channel tile pair (tile t of workgroup y: y, y + nsplit, ...): (tiles_y, tiles_x, n_tiles, nsplit)"""
    Ho, Wo = out_hw(H, W, stride)
    th, tw = tile_fp32(stride)
    tiles_y, tiles_x = _cdiv(Ho, th), _cdiv(Wo, tw)
    n_tiles = B * tiles_y * tiles_x
    pairs = _cdiv(cout, 64) * _cdiv(cin, 64)
    return tiles_y, tiles_x, n_tiles, max(1, min(256 // pairs, 256, n_tiles))


def trips_fp32(B, H, W, cin, cout, stride):
    """tiles every workgroup of a channel tile pair walks, by blockIdx.y"""
    _ty, _tx, n_tiles, nsplit = plan_fp32(B, H, W, cin, cout, stride)
    return [len(range(y, n_tiles, nsplit)) for y in range(nsplit)]


def stage_rows_bf16(stride):
    """output rows of a stage of k_mp_wgrad3x3 (TR): four x rows either way"""
    return 4 if stride == 1 else 2


def plan_bf16(B, H, W, cin, cout, stride):
    """32-column strips; about 256 workgroups by splitting the rows of a strip, with at least two stages (2 TR rows) per split and whole
    stages per split: (n_strips, n_rsplit, rows_per, n_split)"""
    Ho, Wo = out_hw(H, W, stride)
    tr = stage_rows_bf16(stride)
    n_strips = _cdiv(Wo, WG_DW)
    base = B * n_strips * _cdiv(cout, 64) * _cdiv(cin, 64)
    rsplit = max(1, min((256 + base // 2) // base, (Ho + 2 * tr - 1) // (2 * tr)))
    rows_per = _cdiv(_cdiv(Ho, rsplit), tr) * tr
    n_rsplit = _cdiv(Ho, rows_per)
    return n_strips, n_rsplit, rows_per, B * n_strips * n_rsplit


def stages_bf16(B, H, W, cin, cout, stride):
    """stages of every row split of a strip, in split order"""
    Ho, _Wo = out_hw(H, W, stride)
    tr = stage_rows_bf16(stride)
    _ns, n_rsplit, rows_per, _n = plan_bf16(B, H, W, cin, cout, stride)
    return [_cdiv(min(rows_per, Ho - r * rows_per), tr) for r in range(n_rsplit)]


def ring_groups_bf16(stride):
    """x row groups resident in LDS: the copy runs two stages ahead at stride 1, one at stride 2, and a stage reads two groups"""
    return 4 if stride == 1 else 3


# ---------------------------------------------------------------------------------------------------------------------
# case tables: every case names the code path it is there for (checked against the plans by tests/test_wgrad3x3_refs_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------

Case = namedtuple('Case', 'B H W cin cout stride why')

FP32_CASES = [
    Case(1, 1, 1, 8, 8, 1, 'one pixel: only the centre tap is non-zero, the other eight are exactly 0'),
    Case(1, 8, 16, 64, 64, 1, 'exactly one full tile, nsplit 1'),
    Case(1, 9, 17, 4, 4, 1, '2x2 tiles, three of them one row or column wide; one channel quad of one quadrant'),
    Case(2, 16, 32, 72, 40, 1, 'channels not multiples of 64: second ci tile with 8 channels, cout_r padding'),
    Case(4, 24, 48, 256, 256, 1, '16 pairs -> nsplit 16, 36 tiles: three trips for some workgroups, two for others (double buffer wraps, '
                                 'has_next goes false mid-run)'),
    Case(2, 8, 16, 320, 16, 1, 'the head shape: five ci tiles, 48 padded co rows'),
    Case(1, 2, 2, 8, 8, 2, 'one output pixel'),
    Case(2, 18, 34, 64, 64, 2, 'output 9x17: ragged 4x8 tiles in both directions, right and bottom halo inside the map'),
    Case(3, 16, 16, 128, 64, 2, 'two ci tiles at stride 2, batch 3; six tiles over six workgroups, one trip each'),
    Case(3, 32, 32, 256, 256, 2, 'several tiles per workgroup at stride 2: 24 tiles over nsplit 16, two trips for eight workgroups, one for the rest'),
]

BF16_CASES = [
    Case(1, 1, 8, 8, 8, 1, 'fewer rows than one stage (TR = 4), one partial strip'),
    Case(1, 5, 32, 64, 64, 1, 'exactly one strip; TR + 1 rows: a last stage of one row'),
    Case(1, 16, 33, 64, 64, 1, 'second strip of ONE column; n_rsplit = 2 with rows_per 8: halo rows 7/8 cross the row split'),
    Case(2, 12, 31, 72, 40, 1, 'strip one column short; channel blocks of 8 and 40'),
    Case(1, 40, 64, 64, 64, 1, 'five row splits of two stages each, on two full strips: every split but the first and last has both halos in a neighbour'),
    Case(1, 40, 24, 704, 640, 1, 'two row splits of FIVE stages each (110 channel block pairs hold the row split at 2): the x ring of four '
                                 'groups and the dy ring of three wrap, the copy runs two stages ahead'),
    Case(1, 8, 32, 320, 16, 1, 'head shape'),
    Case(1, 2, 2, 8, 8, 2, 'one output pixel, even/odd column store'),
    Case(2, 18, 66, 64, 64, 2, 'output 9x33: odd row count against TR = 2, second strip of one column, parity halves ragged'),
    Case(1, 32, 64, 128, 64, 2, 'row splits at stride 2'),
    Case(1, 32, 48, 704, 640, 2, 'two row splits of four stages each at stride 2: the x ring of three groups wraps'),
]

TABLES = {'fp32': FP32_CASES, 'bf16': BF16_CASES}


def largest(kind):
    """index of the case with the largest workspace: n_split partial tiles of 9 x 64 x 64 per channel block pair, either kernel"""
    def ws(c):
        pairs = _cdiv(c.cout, 64) * _cdiv(c.cin, 64)
        return pairs * (plan_fp32(*c[:6])[3] if kind == 'fp32' else plan_bf16(*c[:6])[3])
    return max(range(len(TABLES[kind])), key=lambda i: ws(TABLES[kind][i]))


def index_of(kind, B, H, W, cin, cout, stride):
    return [tuple(c[:6]) for c in TABLES[kind]].index((B, H, W, cin, cout, stride))


# one-hot placement: (B, H, W, cin, cout, stride) per kernel and stride, eight channels either side (the plans count channel BLOCKS)
PLACE = {
    ('fp32', 1): Case(2, 9, 17, 8, 8, 1, '2x2 tiles of 8x16: boundaries between output rows 7 | 8 and columns 15 | 16'),
    ('fp32', 2): Case(2, 18, 34, 8, 8, 2, 'output 9x17 in 3x3 tiles of 4x8: boundaries 3 | 4 and 7 | 8'),
    ('bf16', 1): Case(2, 16, 33, 8, 8, 1, 'strips 31 | 32, row splits 7 | 8'),
    ('bf16', 2): Case(2, 18, 66, 8, 8, 2, 'output 9x33: strips 31 | 32, row splits 3 | 4'),
}


def place_pixels(kind, stride):
    """[(what, b, oy, ox)]: the four corners, one pixel either side of a boundary of the kernel's pixel decomposition in each direction
    (tiles for fp32, strips and row splits for bf16), one interior pixel; the batch entry alternates"""
    c = PLACE[(kind, stride)]
    Ho, Wo = out_hw(c.H, c.W, stride)
    if kind == 'fp32':
        by, bx = tile_fp32(stride)
    else:
        by, bx = plan_bf16(*c[:6])[2], WG_DW
    assert 0 < by < Ho and 0 < bx < Wo
    px = [('corner', 0, 0), ('corner', 0, Wo - 1), ('corner', Ho - 1, 0), ('corner', Ho - 1, Wo - 1),
          ('above the row boundary', by - 1, 2), ('below the row boundary', by, 2),
          ('left of the column boundary', 1, bx - 1), ('right of the column boundary', 1, bx),
          ('both boundaries, inner side', by - 1, bx - 1), ('both boundaries, outer side', by, bx),
          ('interior', 2, 5)]
    return [(what, i % c.B, oy, ox) for i, (what, oy, ox) in enumerate(px)]


def place_x(kind, stride):
    """arbitrary non-zero floats (bf16-rounded for the bf16 kernel), read-only"""
    c = PLACE[(kind, stride)]
    x = uniform(900 + 2 * stride + (kind == 'bf16'), 1, (c.B, c.H, c.W, c.cin), 0.5, 2.0)
    x = x * np.where(uniform(900 + 2 * stride + (kind == 'bf16'), 2, x.shape) < 0, np.float32(-1), np.float32(1))
    x = bf16_round(x) if kind == 'bf16' else x
    x.setflags(write=False)
    return x


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def make_inputs(kind, seed, shape_x, shape_dy, ints):
    """float variant: uniform in [-1, 1] (bf16-rounded for the bf16 kernel); integer variant: non-zero integers in [-8, 8]"""
    if ints:
        return (np.clip(small_ints(seed, 1, shape_x), -INT_MAX, INT_MAX).astype(np.float32),
                np.clip(small_ints(seed, 3, shape_dy), -INT_MAX, INT_MAX).astype(np.float32))
    x, dy = uniform(seed, 1, shape_x), uniform(seed, 3, shape_dy)
    return (bf16_round(x), bf16_round(dy)) if kind == 'bf16' else (x, dy)


@functools.lru_cache(maxsize=None)
def case_data(kind, i, ints):
    """inputs (float32; what the bf16 kernel gets is exact in bf16) and the reference (dw, S, K) of TABLES[kind][i], computed once and
    read-only"""
    c = TABLES[kind][i]
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    seed = (1000 if kind == 'fp32' else 2000) + 10 * i + (5 if ints else 0)
    x, dy = make_inputs(kind, seed, (c.B, c.H, c.W, c.cin), (c.B, Ho, Wo, c.cout), ints)
    dw, S = wgrad3x3(x, dy, c.stride)
    return _frozen(dict(x=x, dy=dy, dw=dw, S=S, K=c.B * Ho * Wo))
