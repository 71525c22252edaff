"""Plain float64 reference (numpy, no GPU) of the sparse first backbone layer, the occupancy patterns that place its branch points on
purpose, the error scale its float test uses, and the case table its tests share.

  reference, tile_tap_counts    pcp_sparse_conv3x3_s2 / pcp_mp_sparse_conv3x3_s2: k_sparse_conv_s2                  (csrc/sparseconv.hip)

The operation is ZeroPad2d(1) + Conv2d(64, cout, 3, stride 2) + bias (+ ReLU) on the canvas that holds pillar row p at the cell
voxel_coords[p] = [b, 0, y, x] and zeros elsewhere; the kernel never sees that canvas, it walks the pillar list through the pillariser's
cell -> rank table.  reference() scatters the rows and calls mp_forward_refs.conv3x3: (y, S), S = sum |x||w| + |b|.

What the kernel branches on is the occupancy, not the values: per (frame, 8 x 16-pixel output tile, tap) the number of in-range pixels of
the tile that read an occupied cell through the tap ("rows"), in chunks ("items") of 32, row tiles of 16 inside an item, the two 64-pixel
halves of the tile whose counts the compaction joins, and items walked four at a time with two tail stages.  tile_tap_counts() restates
that geometry (iy = 2 oy + ky - 1, ix = 2 ox + kx - 1, tap = 3 ky + kx, output (ny - 1) // 2 + 1 by (nx - 1) // 2 + 1) so that
tests/test_sparse_conv_refs_cpu.py can assert which counts the table reaches.  A cell feeds at most four (pixel, tap) pairs, decided by its
parity: (even y, even x) tap 4 of one pixel; (odd, even) taps 1 and 7 of two pixels; (even, odd) taps 3 and 5; (odd, odd) taps 0, 2, 6, 8 of
four pixels -- first_k_of_class places exactly k rows of tap 4 (or of the last tap of another class) into one tile.

The bar of the float cases, element by element against float64, nothing on top: bound(S, BAR_K) = (BAR_K + 2) 2^-24 S with
BAR_K = 9 * 64 + 9 + 1: the 576 products of a pixel, at most nine additions of a tap's product block into the pixel's accumulator in LDS
(the matrix unit sums the 64 products of a block, the block is then added as one term), and the bias.  pointwise_refs states the rule: every
multiplication and addition rounds once, relative 2^-24, and a term passes through at most K + 2 of them.

Integer cases: pillar rows and weights hold non-zero integers in [-8, 8] (mp_forward_refs.ints8), the bias non-zero integers in [-8, 8].
S <= 9 * 64 * 64 + 8 < 2^22, so every product and every partial sum is an integer below 2^24, exact in fp32 in any order: a correct kernel
owes the float64 result bit for bit.  They see every dropped or doubled row, wrong tap and transposed index and are blind to lost precision;
the float cases (rows uniform in [-1, 1], weights in [-0.05, 0.05]) are there for that.

Points.  points_for() puts one to three points at the centre of every occupied cell of a grid whose origin is 0 and whose voxel is 0.25:
centres (i + 0.5) / 4 and the pillariser's floor((x - 0) / 0.25) are exact in fp32, so the pillar set is the pattern, cell for cell.
"""
import functools
from collections import namedtuple

import numpy as np

from mp_forward_refs import conv3x3, ints8, out_hw
from pointwise_refs import bound, f64, uniform

TH, TW = 8, 16                   # output pixels per workgroup of k_sparse_conv_s2: 8 rows by 16 columns
CHUNK = 32                       # rows per item
CIN = 64
BAR_K = 9 * CIN + 9 + 1          # products, block additions, bias (module docstring)
EXACT = 2.0 ** 22                # integer cases: max S below this
VOXEL = 0.25                     # a power of two: cell centres and the pillariser's division are exact
Z_RANGE = (-2.0, 2.0)

GridSpec = namedtuple('GridSpec', 'nx ny batch')


def pc_range(g):
    return [0.0, 0.0, Z_RANGE[0], g.nx * VOXEL, g.ny * VOXEL, Z_RANGE[1]]


def voxel_size(_g):
    return [VOXEL, VOXEL, Z_RANGE[1] - Z_RANGE[0]]


def grid_size(g):
    return [g.nx, g.ny, 1]


# ---------------------------------------------------------------------------------------------------------------------
# occupancy patterns: (B, ny, nx) -> bool map.  A pattern is a tuple (kind, arguments ...)
# ---------------------------------------------------------------------------------------------------------------------

def _tile_pixels(ny, nx, tile):
    """the in-range output pixels (oy, ox) of tile (tile row, tile column), in the kernel's pixel order"""
    ho, wo = out_hw(ny, nx, 2)
    ty, tx = tile
    return [(oy, ox) for oy in range(ty * TH, min(ty * TH + TH, ho)) for ox in range(tx * TW, min(tx * TW + TW, wo))]


def empty():
    return ('empty',)


def single(y, x):
    return ('single', y, x)


def full():
    return ('full',)


def full_but(*cells):
    """everything but the listed cells (y, x)"""
    return ('full_but',) + tuple(cells)


def checker(py, px):
    """only the cells of one parity class: y % 2 == py and x % 2 == px"""
    return ('checker', py, px)


def first_k_of_class(tile, parity, k):
    """exactly k cells of the class (y % 2, x % 2) = parity inside the input footprint of one output tile: the cells (2 oy + py, 2 ox + px) of
    its first k pixels in pixel order that have such a cell inside the map (py = 0: read through ky = 1; py = 1: through ky = 2 -- and
    through ky = 0 by the pixel below; the same along x)"""
    return ('first_k', tuple(tile), tuple(parity), k)


def wave1_only(tile):
    """every cell whose readers all lie in pixels 64..127 of the tile (its rows 4..7): the first half's count is 0 for every tap"""
    return ('rows', tuple(tile), 4, 7)


def wave0_only(tile):
    """the mirror: every cell whose readers all lie in pixels 0..63 (rows 0..3)"""
    return ('rows', tuple(tile), 0, 3)


def uniform_density(p, seed):
    """every cell occupied with probability p, every frame on its own"""
    return ('uniform', p, seed)


def per_batch(*patterns):
    """one pattern per frame"""
    return ('per_batch',) + tuple(patterns)


def union(*patterns):
    return ('union',) + tuple(patterns)


def _occ(pattern, B, ny, nx):
    kind = pattern[0]
    occ = np.zeros((B, ny, nx), bool)
    if kind == 'empty':
        pass
    elif kind == 'single':
        occ[:, pattern[1], pattern[2]] = True
    elif kind == 'full':
        occ[:] = True
    elif kind == 'full_but':
        occ[:] = True
        for y, x in pattern[1:]:
            occ[:, y, x] = False
    elif kind == 'checker':
        occ[:, pattern[1]::2, pattern[2]::2] = True
    elif kind == 'first_k':
        _kind, tile, (py, px), k = pattern
        cells = [(2 * oy + py, 2 * ox + px) for oy, ox in _tile_pixels(ny, nx, tile) if 2 * oy + py < ny and 2 * ox + px < nx]
        assert len(cells) >= k, 'tile %s has %d cells of class %s, asked for %d' % (tile, len(cells), (py, px), k)
        for y, x in cells[:k]:
            occ[:, y, x] = True
    elif kind == 'rows':
        _kind, (ty, tx), r0, r1 = pattern
        ho, wo = out_hw(ny, nx, 2)
        assert ty * TH + r1 < ho
        # cell rows 2 (oy0 + r0) .. 2 (oy0 + r1): read by output rows oy0 + r0 .. oy0 + r1 only (the odd rows on either side have a second reader)
        y0, y1 = 2 * (ty * TH + r0), 2 * (ty * TH + r1)
        x0, x1 = 2 * tx * TW, 2 * (min(tx * TW + TW, wo) - 1)             # the same along x: no reader in a neighbouring tile
        occ[:, y0:y1 + 1, x0:x1 + 1] = True
    elif kind == 'uniform':
        occ[:] = f64(uniform(pattern[2], 1, (B, ny, nx), 0.0, 1.0)) < pattern[1]
    elif kind == 'per_batch':
        assert len(pattern) - 1 == B
        for b, sub in enumerate(pattern[1:]):
            occ[b] = _occ(sub, 1, ny, nx)[0]
    elif kind == 'union':
        for sub in pattern[1:]:
            occ |= _occ(sub, B, ny, nx)
    else:
        raise ValueError(pattern)
    return occ


def occupancy(case):
    """the boolean (B, ny, nx) map of a case"""
    return _occ(case.pattern, case.B, case.ny, case.nx)


def coords_of(occ):
    """the pillar list of an occupancy map in the pillariser's order (ascending frame, x, y), as its voxel_coords rows [b, 0, y, x]: (P, 4) int32"""
    b, x, y = np.nonzero(occ.transpose(0, 2, 1))
    return np.stack([b, np.zeros_like(b), y, x], 1).astype(np.int32)


def points_for(occ, grid, seed=1):
    """(N, 5) float32 rows [frame, x, y, z, intensity]: one to three points at the centre of every occupied cell, z inside the range,
    shuffled by a fixed seed"""
    assert occ.shape == (grid.batch, grid.ny, grid.nx)
    rs = np.random.RandomState(4200 + seed)
    b, y, x = np.nonzero(occ)
    rep = rs.randint(1, 4, size=b.shape[0])
    b, y, x = np.repeat(b, rep), np.repeat(y, rep), np.repeat(x, rep)
    pts = np.zeros((b.shape[0], 5), np.float32)
    pts[:, 0] = b
    pts[:, 1] = (x + 0.5) * VOXEL
    pts[:, 2] = (y + 0.5) * VOXEL
    pts[:, 3] = rs.randint(-3, 4, size=b.shape[0]) * 0.5                   # -1.5 .. 1.5
    pts[:, 4] = rs.randint(0, 256, size=b.shape[0]) / 256.0
    return np.ascontiguousarray(pts[rs.permutation(pts.shape[0])])


def cells_of_points(pts, grid):
    """the pillariser's row -> cell arithmetic in float32: floor((p - min) / voxel) with min = 0, rows outside the range dropped: the
    boolean (B, ny, nx) map of the cells that hold a point"""
    pts = np.asarray(pts, np.float32)
    v = np.float32(VOXEL)
    cx, cy = np.floor((pts[:, 1] - np.float32(0)) / v), np.floor((pts[:, 2] - np.float32(0)) / v)
    assert cx.dtype == np.float32
    ok = (cx >= 0) & (cx < grid.nx) & (cy >= 0) & (cy < grid.ny) & (pts[:, 0] >= 0) & (pts[:, 0] < grid.batch)
    occ = np.zeros((grid.batch, grid.ny, grid.nx), bool)
    occ[pts[ok, 0].astype(np.int64), cy[ok].astype(np.int64), cx[ok].astype(np.int64)] = True
    return occ


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's geometry, restated
# ---------------------------------------------------------------------------------------------------------------------

TapCounts = namedtuple('TapCounts', 'count lo hi items pixel_taps')


def tile_tap_counts(occ):
    """count[b, tile row, tile column, tap]: how many in-range output pixels of the tile read an occupied cell through the tap; lo / hi: the
    same within pixels 0..63 / 64..127 of the tile; items[b, tile row, tile column] = sum over taps of ceil(count / 32); pixel_taps[b, oy, ox]:
    the number of taps through which the pixel reads an occupied cell"""
    B, ny, nx = occ.shape
    ho, wo = out_hw(ny, nx, 2)
    ty, tx = -(-ho // TH), -(-wo // TW)
    fed = np.zeros((B, ty * TH, tx * TW, 9), bool)
    oy, ox = np.arange(ho), np.arange(wo)
    for t in range(9):
        iy, ix = 2 * oy + t // 3 - 1, 2 * ox + t % 3 - 1
        vy, vx = (iy >= 0) & (iy < ny), (ix >= 0) & (ix < nx)
        sub = occ[:, np.clip(iy, 0, ny - 1)][:, :, np.clip(ix, 0, nx - 1)]
        fed[:, :ho, :wo, t] = sub & vy[None, :, None] & vx[None, None, :]
    f = fed.reshape(B, ty, TH, tx, TW, 9)
    count = f.sum((2, 4))
    return TapCounts(count, f[:, :, :TH // 2].sum((2, 4)), f[:, :, TH // 2:].sum((2, 4)), (-(-count // CHUNK)).sum(-1),
                     fed[:, :ho, :wo].sum(-1))


def reference(occ, coords, pf, w, b, relu):
    """the layer in float64 from the pillar list: pf[p] scattered to canvas[b, y, x] for coords[p] = [b, 0, y, x] (rows of pf past len(coords)
    are not read), then mp_forward_refs.conv3x3 at stride 2: (y, S).  The pillar list must be the occupancy map, each cell once"""
    coords = np.asarray(coords)
    B, ny, nx = occ.shape
    P = coords.shape[0]
    assert coords.shape == (P, 4) and pf.shape[0] >= P and pf.shape[1] == CIN
    seen = np.zeros_like(occ)
    seen[coords[:, 0], coords[:, 2], coords[:, 3]] = True
    assert P == int(occ.sum()) and np.array_equal(seen, occ) and not coords[:, 1].any()
    canvas = np.zeros((B, ny, nx, CIN), np.float64)
    canvas[coords[:, 0], coords[:, 2], coords[:, 3]] = f64(pf[:P])
    return conv3x3(canvas, w, b, 2, relu)


def canvas_of(occ, coords, pf):
    """the float64 canvas alone (the CPU test hands it to torch)"""
    canvas = np.zeros(occ.shape + (CIN,), np.float64)
    canvas[coords[:, 0], coords[:, 2], coords[:, 3]] = f64(pf[:coords.shape[0]])
    return canvas


def one_hot_weights(tap):
    """w[n, c, ky, kx] = 1 where n == c and 3 ky + kx == tap, else 0: (64, 64, 3, 3) float32"""
    w = np.zeros((CIN, CIN, 3, 3), np.float32)
    w[np.arange(CIN), np.arange(CIN), tap // 3, tap % 3] = 1.0
    return w


def one_hot_expect(occ, coords, pf, tap):
    """what one_hot_weights(tap) makes of the pillar list, by lookup and without any sum: out[b, oy, ox] = pf[rank of the cell
    (2 oy + ky - 1, 2 ox + kx - 1)], or 0 where that cell is empty or outside the map: (B, ho, wo, 64), the dtype of pf"""
    B, ny, nx = occ.shape
    ho, wo = out_hw(ny, nx, 2)
    rank = np.full((B, ny, nx), -1, np.int64)
    rank[coords[:, 0], coords[:, 2], coords[:, 3]] = np.arange(coords.shape[0])
    out = np.zeros((B, ho, wo, CIN), pf.dtype)
    for b in range(B):
        for oy in range(ho):
            for ox in range(wo):
                iy, ix = 2 * oy + tap // 3 - 1, 2 * ox + tap % 3 - 1
                if 0 <= iy < ny and 0 <= ix < nx and rank[b, iy, ix] >= 0:
                    out[b, oy, ox] = pf[rank[b, iy, ix]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case table: every case names the branch point it is there for (tests/test_sparse_conv_refs_cpu.py asserts the counts)
# ---------------------------------------------------------------------------------------------------------------------

Case = namedtuple('Case', 'name B nx ny pattern cout')
EE, OE, EO, OO = (0, 0), (1, 0), (0, 1), (1, 1)             # parity classes (y % 2, x % 2)

CASES = [
    # nx = 36, ny = 20: 10 x 18 outputs, partial last tile in both directions (16-, 32- and 4-pixel tiles), nx > ny
    Case('wide_empty', 2, 36, 20, empty(), 64),
    Case('wide_full', 1, 36, 20, full(), 64),
    Case('wide_single_corner', 1, 36, 20, single(19, 35), 32),
    Case('wide_checker_ee', 2, 36, 20, checker(0, 0), 64),
    Case('wide_checker_oe', 1, 36, 20, checker(1, 0), 64),
    Case('wide_density_05_005', 3, 36, 20, per_batch(uniform_density(0.5, 11), uniform_density(0.05, 12), uniform_density(0.5, 13)), 64),
    Case('wide_edge_tile_15_16', 2, 36, 20, per_batch(first_k_of_class((0, 1), EE, 15), first_k_of_class((0, 1), EE, 16)), 64),
    # (even, odd) cells: k rows of tap 5 and k - (those in the tile's last column) of tap 3; (odd, odd): four taps
    Case('wide_items_5_6_7', 3, 36, 20, per_batch(first_k_of_class((0, 0), EO, 65), first_k_of_class((0, 0), OO, 33),
                                                  first_k_of_class((0, 0), EO, 97)), 64),
    # nx = 20, ny = 36: the transpose, 18 x 10 outputs, three tile rows of one ragged tile each, nx < ny
    Case('tall_full', 1, 20, 36, full(), 64),
    Case('tall_checker_oo', 2, 20, 36, checker(1, 1), 64),
    Case('tall_checker_eo', 1, 20, 36, checker(0, 1), 32),
    Case('tall_density_05', 2, 20, 36, uniform_density(0.5, 21), 64),
    Case('tall_density_005', 3, 20, 36, uniform_density(0.05, 22), 64),
    Case('tall_17_31_33', 3, 20, 36, per_batch(first_k_of_class((1, 0), EE, 17), first_k_of_class((1, 0), EE, 31),
                                               first_k_of_class((1, 0), EE, 33)), 64),
    # nx = 33, ny = 17: both odd, 9 x 17 outputs, the last tap row and column outside the map
    Case('odd_full', 2, 33, 17, full(), 64),
    Case('odd_density_05', 2, 33, 17, uniform_density(0.5, 31), 64),
    Case('odd_checker_oo', 1, 33, 17, checker(1, 1), 64),
    Case('odd_last_row_and_column', 1, 33, 17, union(('rows', (1, 0), 0, 0), single(3, 32), single(8, 32)), 64),
    # nx = 64, ny = 32: 16 x 32 outputs, 2 x 2 whole tiles
    Case('whole_full', 2, 64, 32, full(), 64),
    Case('whole_full_but_one', 1, 64, 32, full_but((20, 40)), 64),
    Case('whole_1_32_128', 3, 64, 32, per_batch(first_k_of_class((1, 1), EE, 1), first_k_of_class((1, 1), EE, 32),
                                                first_k_of_class((1, 1), EE, 128)), 64),
    Case('whole_63_64_65', 3, 64, 32, per_batch(first_k_of_class((0, 1), EE, 63), first_k_of_class((0, 1), EE, 64),
                                                first_k_of_class((0, 1), EE, 65)), 64),
    Case('whole_96_97_127', 3, 64, 32, per_batch(first_k_of_class((1, 0), EE, 96), first_k_of_class((1, 0), EE, 97),
                                                 first_k_of_class((1, 0), EE, 127)), 64),
    Case('whole_mixed_classes', 3, 64, 32, per_batch(union(first_k_of_class((0, 0), OE, 20), first_k_of_class((0, 1), OE, 40),
                                                          first_k_of_class((1, 0), OO, 20), first_k_of_class((1, 1), EO, 70)),
                                                    union(first_k_of_class((0, 0), OO, 40), first_k_of_class((1, 1), OO, 60)),
                                                    union(first_k_of_class((0, 1), OE, 100), first_k_of_class((1, 0), EO, 33))), 64),
    Case('whole_wave1_only', 2, 64, 32, per_batch(wave1_only((0, 1)), wave1_only((1, 0))), 64),
    Case('whole_wave0_only', 2, 64, 32, per_batch(wave0_only((1, 1)), wave0_only((0, 0))), 64),
    Case('whole_density_05_005', 2, 64, 32, per_batch(uniform_density(0.5, 41), uniform_density(0.05, 42)), 64),
    Case('whole_mixed_cout_32', 2, 64, 32, per_batch(uniform_density(0.5, 43), checker(1, 1)), 32),
    # the smallest grids
    Case('one_cell', 1, 1, 1, full(), 64),
    Case('two_columns_full', 1, 2, 31, full(), 64),
    Case('two_columns_density_05', 3, 2, 31, uniform_density(0.5, 51), 64),
]
CASE_INDEX = {c.name: i for i, c in enumerate(CASES)}
assert len(CASE_INDEX) == len(CASES)

COUTS = (4, 12, 20, 32, 48, 60, 64)
COUT_CASE = 'wide_density_05_005'                      # mixed occupancy on a grid with partial tiles
WIDE_ROW_CASE, WIDE_ROW_COUTS, WIDE_ROW_PAD, FILL = 'wide_density_05_005', (20, 64), 12, 7.0
ONE_HOT_CASES = ('wide_density_05_005', 'tall_density_05', 'odd_density_05')
BF16_CASES = ('wide_density_05_005', 'odd_full', 'whole_96_97_127')
OTHER_PILLARISER_CASE = 'tall_density_05'


def grid_of(case):
    return GridSpec(case.nx, case.ny, case.B)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def inputs(i, variant, P, cout):
    """(pf (P, 64), w (cout, 64, 3, 3), b (cout,)) float32 of CASES[i]: 'ints' | 'float'"""
    seed = 8000 + 2 * i + (1 if variant == 'float' else 0)
    rows = max(P, 1)
    if variant == 'float':
        return uniform(seed, 1, (rows, CIN))[:P], uniform(seed, 2, (cout, CIN, 3, 3), -0.05, 0.05), uniform(seed, 3, (cout,), -0.2, 0.2)
    return ints8(seed, 1, (rows, CIN))[:P], ints8(seed, 3, (cout, CIN, 3, 3)), ints8(seed, 5, (cout,))


@functools.lru_cache(maxsize=None)
def case_data(i, variant, cout=None):
    """occupancy, the pillar list in the pillariser's order, inputs (float32) and the reference of CASES[i], computed once and read-only.
    pre is the value before the ReLU, bar the element-wise tolerance of the float variant (None for 'ints').  cout overrides the case's"""
    c = CASES[i]
    cout = cout or c.cout
    occ = occupancy(c)
    coords = coords_of(occ)
    pf, w, b = inputs(i, variant, coords.shape[0], cout)
    pre, S = reference(occ, coords, pf, w, b, False)
    return _frozen(dict(occ=occ, coords=coords, pf=pf, w=w, b=b, pre=pre, S=S, bar=bound(S, BAR_K) if variant == 'float' else None))
