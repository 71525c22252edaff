"""Plain float64 references (numpy, no GPU) of the fp32 3x3 forward convolutions, the two error scales their tests use, the integer inputs
on which every correct fp32 evaluation owes the same bits, and the case tables those tests share.

  direct            pcp_conv3x3: k_conv3x3 (strides 1 and 2) and k_conv3x3_s2w (option conv_s2_form)                 (csrc/conv.hip)
  F(2x2, 3x3)       pcp_conv3x3_winograd (k_wino) and pcp_conv3x3_winograd_ws                          (csrc/wino.hip, csrc/wino_ws.hip)
  F(4x4, 3x3)       pcp_conv3x3_winograd4 (through memory) and the fused k_wino4f / k_wino4h / k_wino4c   (csrc/wino4*.hip, wino4_common.h)
  bf16x3            pcp_conv3x3_bf16x3, the opt-in three-term bf16 split                                         (csrc/conv_bf16x3.hip)

The convolution itself and its scale S = sum |x||w| + |b| are mp_forward_refs.conv3x3; maps are NHWC, weights (cout, cin, 3, 3).

The bars, element by element against float64, nothing on top (pointwise_refs.bound(S, K) = (K + 2) 2^-24 S):

  direct    bound(S, 9 cin + 1): 9 cin products and the bias, the rule pointwise_refs states for the fp32 matrix unit.
  Winograd  bound(T, cin + 16) with the Winograd scale T of wino_scale():
                T = |A^T| ( sum_c |U_c| (.) (|B^T| |d_c| |B|) ) |A| + |b|
            U the fp32-rounded filter transform of pcp_amd/pack.py, d_c the zero-padded patch of the tile that owns the pixel.  Every
            rounding of the evaluation acts on a partial result whose magnitude T bounds, so the error is at most (number of roundings
            on the longest path) 2^-24 T.  The longest path, counted from the kernels: the input transform rounds at most 3 times per
            pass (t[0] = 4 d0 - 5 d2 + d4 of bt6 in csrc/wino4.hip and csrc/wino4f.hip without contraction; 2 with the explicit fmas of
            wino4_common.h; 1 for F(2x2), whose B^T rows are differences), U is rounded once, the output transform rounds at most 3
            times per pass (y[3] = d12 + 8 d34 + m5 of at6 / at6v; 2 for F(2x2)): 6 + 1 + 6 = 13 <= 16.  The cin accumulations, the
            multiplication and the bias add are the cin + 2 of bound().
  bf16x3    bound(S, 9 cin + 1) + B3_RESIDUAL (S - |b|).  The split of csrc/conv_bf16x3.hip: hi = bf16(x) (nearest even, |x - hi| <=
            2^-9 |x|), lo = bf16(x - hi) (x - hi is exact in fp32), so x = hi + lo + e with |e| <= 2^-18 |x| and |lo| <= 2^-9 (1 +
            2^-9) |x|; the same for w.  The kernel adds hi_x hi_w + hi_x lo_w + lo_x hi_w, each product exact in the fp32 accumulator;
            what it leaves out of x w is lo_x lo_w + e_x w + (x - e_x) e_w, at most 3 * 2^-18 (1 + 2^-8) |x||w| = B3_RESIDUAL |x||w|.
            The fp32 term stays that of the direct kernel: the accumulator passes through 27 cin / 16 matrix instructions of 16 exact
            products each, so (9 cin + 3) half-ulp roundings allow more than five per instruction.

Integer inputs.  Direct kernels and bf16x3: non-zero integers in [-8, 8] (mp_forward_refs.ints8), integer bias; every partial sum is an
integer below 2^24 in any order (the CPU test asserts max S < 2^22), and the values are exact bf16, so the low terms of the split are 0.
Winograd kernels: maps from {0, +-1, +-2} at density 1/2 ({0, +-1} above 384 input channels), weights from 9 * {0, +-1} at density 1/2
(1/4 above 384 input channels), bias a non-zero multiple of 1/4.  With weights that are multiples of 9, G g G^T has only powers of two in
its denominators (1/64 for F(4x4), 1/4 for F(2x2)), so U is exact in fp32; V = B^T d B is an integer; every product and partial sum is a
multiple of 2^-6, and the integer-coefficient output transform is exact while magnitudes stay below 2^24 2^-6.  wino_headroom() returns
the two magnitudes that must stay below that, in units of 2^-6; a case may be in a Winograd table only if both are below 0.5 * 2^24 (a
condition, asserted by tests/test_conv3x3_refs_cpu.py for every case).  One thing pack.py adds: its float64 G g G^T sums terms +-9
fl(1/6)^2 whose partial sums round, so where the exact U is 0 the packed F(4x4) U may hold a residue of about 2^-53 instead.  A residue
cannot change a bit: what all residues together add to any intermediate stays below 2^-31 (the third figure of wino_headroom, asserted per
case), a quarter of the fp32 spacing at 2^-6, so every operation whose exact result is a non-zero multiple of 2^-6 still rounds to it, and
an exact 0 that became a residue is absorbed by the final add of the non-zero bias.  Integer cases see every indexing, padding, packing
and ordering mistake at any magnitude and are blind to lost precision; uniform maps in [-1, 1] with weights in [-0.05, 0.05] are there for
that.
"""
import functools
from collections import namedtuple

import numpy as np

from mp_forward_refs import conv3x3, ints8, out_hw, taps_inside  # noqa: F401  (the tests reach them through this module)
from pcp_amd.pack import _WINO4_G, _WINO_G
from pointwise_refs import bound, f64, uniform

B3_RESIDUAL = 3.0 * 2.0 ** -18 * (1.0 + 2.0 ** -8)
WINO_ROUNDINGS = 16              # the issue's count of the transform roundings; the kernels' longest path has 13 (module docstring)
EXACT_DIRECT = 2.0 ** 22         # integer cases of the direct kernels: max S below this
EXACT_WINO = 0.5 * 2.0 ** 24     # integer cases of the Winograd kernels: both magnitudes of wino_headroom below this, in units of 2^-6

# the transforms, restated from the kernels' comments: F(2x2, 3x3) on points 0, +-1, inf; F(4x4, 3x3) (Lavin & Gray) on 0, +-1, +-2, inf
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
WINO = {2: (BT2, AT2, np.array(_WINO_G, np.float64)), 4: (BT4, AT4, np.array(_WINO4_G, np.float64))}


# ---------------------------------------------------------------------------------------------------------------------
# Winograd: filter transform, patches, the scale T, the exactness headroom
# ---------------------------------------------------------------------------------------------------------------------

def wino_u(w, m):
    """U = G g G^T in float64, rounded once to fp32 (pack.py's arithmetic): (cout, cin, m + 2, m + 2) float32"""
    G = WINO[m][2]
    return np.einsum('ia,ncab,jb->ncij', G, f64(w), G).astype(np.float32)


def wino_patches(x, m, pad_mode='constant'):
    """the (m + 2) x (m + 2) input patch of every m x m output tile, tiles anchored at pixel (0, 0), zero outside the map:
    (B, tiles_y, tiles_x, m + 2, m + 2, cin), the dtype of x.  pad_mode 'edge' is the planted error of a border that is not zeroed"""
    B, H, W, C = x.shape
    ty, tx = -(-H // m), -(-W // m)
    xp = np.pad(x, ((0, 0), (1, ty * m + 1 - H), (1, tx * m + 1 - W), (0, 0)), mode=pad_mode)
    d = np.empty((B, ty, tx, m + 2, m + 2, C), x.dtype)
    for r in range(m + 2):
        for s in range(m + 2):
            d[:, :, :, r, s, :] = xp[:, r:r + ty * m:m, s:s + tx * m:m, :]
    return d


def wino_untile(yt, H, W):
    """(B, tiles_y, tiles_x, m, m, cout) -> (B, H, W, cout): the tiles side by side, cropped to the map"""
    B, ty, tx, m, _m, N = yt.shape
    return np.ascontiguousarray(yt.transpose(0, 1, 3, 2, 4, 5).reshape(B, ty * m, tx * m, N)[:, :H, :W, :])


def _position_sums(V, U):
    """sum_c V[..., i, j, c] U[n, c, i, j]: (B, ty, tx, n, n, cout)"""
    n = V.shape[3]
    out = np.empty(V.shape[:5] + (U.shape[0],))
    for i in range(n):
        for j in range(n):
            out[:, :, :, i, j, :] = V[:, :, :, i, j, :] @ U[:, :, i, j].T
    return out


def _through(mat, M):
    return np.einsum('pi,btuijn,qj->btupqn', mat, M, mat)


def wino_scale(x, w, b, m):
    """T = |A^T| ( sum_c |U_c| (.) (|B^T| |d_c| |B|) ) |A| + |b| per output element: (B, H, W, cout)"""
    BT, AT = np.abs(WINO[m][0]), np.abs(WINO[m][1])
    Vb = np.einsum('ir,btursc,js->btuijc', BT, np.abs(wino_patches(f64(x), m)), BT)
    return wino_untile(_through(AT, _position_sums(Vb, np.abs(f64(wino_u(w, m))))), x.shape[1], x.shape[2]) + np.abs(f64(b))


def wino_headroom(x, w, m, u_packed=None):
    """the exactness condition of an integer case, in units of 2^-6: (max sum_c |U_c||V_c| -- no partial sum in any order exceeds it --,
    max |A^T| |M| |A| with M = sum_c U_c V_c -- no intermediate of the output transform exceeds it).  With u_packed, the (cout, cin, n, n)
    filter transform a pack function really made, a third figure in plain units: max |A^T| (sum_c |u_packed - U|_c |V_c|) |A|, what
    the pack's residues where U is 0 (module docstring) can add to any intermediate"""
    BT, AT = WINO[m][0], np.abs(WINO[m][1])
    U = f64(wino_u(w, m))
    V = np.einsum('ir,btursc,js->btuijc', BT, wino_patches(f64(x), m), BT)
    out = (64.0 * float(_position_sums(np.abs(V), np.abs(U)).max()), 64.0 * float(_through(AT, np.abs(_position_sums(V, U))).max()))
    if u_packed is not None:
        out += (float(_through(AT, _position_sums(np.abs(V), np.abs(f64(u_packed) - U))).max()),)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the Winograd pipelines (for the CPU test: the references can see planted mistakes)
# ---------------------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def _bt(d, m):
    """B^T along axis 0 in fp32, the operations of bt6 (wino4_common.h) / the differences of F(2x2)"""
    if m == 2:
        return np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]])
    p, q = _fma(np.float32(-4), d[2], d[4]), _fma(np.float32(-4), d[1], d[3])
    r, s = d[4] - d[2], np.float32(2) * (d[3] - d[1])
    return np.stack([_fma(np.float32(4), d[0], _fma(np.float32(-5), d[2], d[4])), p + q, p - q, r + s, r - s,
                     _fma(np.float32(4), d[1], _fma(np.float32(-5), d[3], d[5]))])


def _at(v, m):
    """A^T along axis 0 in fp32, the operations of at6v"""
    if m == 2:
        return np.stack([(v[0] + v[1]) + v[2], (v[1] - v[2]) - v[3]])
    s12, d12, s34, d34 = v[1] + v[2], v[1] - v[2], v[3] + v[4], v[3] - v[4]
    return np.stack([(v[0] + s12) + s34, _fma(np.float32(2), d34, d12), _fma(np.float32(4), s34, s12),
                     _fma(np.float32(8), d34, d12) + v[5]])


PLANTS = ('drop_tap', 'mirror_kx', 'skip_slice', 'border')


def wino_emulate(x, w, b, m, reverse=False, plant=None):
    """the Winograd evaluation in fp32 numpy: V = B^T d B, M = sum_c U_c V_c one channel after the other (reverse: from the last channel
    down), Y = A^T M A + b; no ReLU.  plant: one of PLANTS --
      drop_tap    the last tile of the map (ragged where the map is) runs without the filter tap (ky, kx) = (0, 0)
      mirror_kx   the filter taps are read with kx mirrored
      skip_slice  the last eight input channels are never accumulated
      border      the halo outside the map holds the edge pixels, not zeros"""
    x, w, b = np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(b, np.float32)
    assert plant is None or plant in PLANTS
    cin = x.shape[-1]
    U = wino_u(w[..., ::-1] if plant == 'mirror_kx' else w, m)
    d = wino_patches(x, m, 'edge' if plant == 'border' else 'constant')                # (B, ty, tx, n, n, C)
    V = _bt(np.moveaxis(d, 3, 0), m)                                                    # rows:    (i, B, ty, tx, s, C)
    V = _bt(np.moveaxis(V, 4, 0), m)                                                    # columns: (j, i, B, ty, tx, C)
    V = np.ascontiguousarray(V.transpose(2, 3, 4, 1, 0, 5))                             # (B, ty, tx, i, j, C)
    chans = list(range(cin - 8 if plant == 'skip_slice' else cin))
    if reverse:
        chans.reverse()

    def products(V, U):
        M = np.zeros(V.shape[:5] + (U.shape[0],), np.float32)
        Ut = np.ascontiguousarray(U.transpose(1, 2, 3, 0))                              # (C, i, j, N)
        for c in chans:
            M += V[..., c, None] * Ut[c]
        return M
    M = products(V, U)
    if plant == 'drop_tap':
        w0 = w.copy()
        w0[:, :, 0, 0] = 0
        M[-1, -1, -1] = products(V[-1:, -1:, -1:], wino_u(w0, m))[0, 0, 0]
    Y = _at(np.moveaxis(M, 3, 0), m)                                                    # (p, B, ty, tx, j, N)
    Y = _at(np.moveaxis(Y, 4, 0), m)                                                    # (q, p, B, ty, tx, N)
    return wino_untile(Y.transpose(2, 3, 4, 1, 0, 5), x.shape[1], x.shape[2]) + b


# ---------------------------------------------------------------------------------------------------------------------
# input generators
# ---------------------------------------------------------------------------------------------------------------------

def sparse_ints(seed, col, shape, mags, density):
    """0 with probability 1 - density, else +-(one of mags), float32"""
    live = f64(uniform(seed, col, shape, 0.0, 1.0)) < density
    pick = np.minimum(np.floor(f64(uniform(seed, col + 1, shape, 0.0, float(len(mags))))), len(mags) - 1).astype(np.int64)
    sign = np.where(uniform(seed, col + 2, shape) < 0, -1.0, 1.0)
    return np.where(live, np.asarray(mags, np.float64)[pick] * sign, 0.0).astype(np.float32)


def wino_int_inputs(seed, shape_x, shape_w):
    """the Winograd integer inputs of the module docstring: (x, w, b)"""
    wide = shape_x[-1] > 384
    x = sparse_ints(seed, 1, shape_x, (1.0,) if wide else (1.0, 2.0), 0.5)
    w = sparse_ints(seed, 4, shape_w, (9.0,), 0.25 if wide else 0.5)
    k = np.clip(np.floor(f64(uniform(seed, 7, (shape_w[0],), 1.0, 33.0))), 1, 32) * np.where(uniform(seed, 8, (shape_w[0],)) < 0, -1.0, 1.0)
    b = (k / 4.0).astype(np.float32)                                                   # never 0: the last add absorbs a residue
    return x, w, b


# ---------------------------------------------------------------------------------------------------------------------
# case tables: the smallest shapes at which each kernel can still go wrong; every case runs with ReLU off and on
# ---------------------------------------------------------------------------------------------------------------------

Case = namedtuple('Case', 'cin cout B H W stride why')

_MAPS = [((1, 16, 16), 'whole tiles'), ((2, 17, 23), 'odd map of two frames: ragged last row and column, right and bottom halo outside'),
         ((1, 33, 9), 'narrower than a tile, five tile rows')]
_CINS = [(16, 'one slice'), (64, 'four slices: the double buffer wraps')]
_COUTS = [(32, 'cout_pad 32: the 32-channel tile'), (64, 'one 64-channel tile'), (100, 'padded channels'),
          (192, 'cout_pad % 128 != 0: three 64-channel tiles')]


def _direct(stride):
    return [Case(cin, cout, B, H, W, stride, '%s; %s; %s' % (mw, kw, nw)) for (B, H, W), mw in _MAPS for cin, kw in _CINS for cout, nw in _COUTS]


TABLES = {
    'direct_s1': _direct(1),
    'direct_s2': _direct(2),
    'wino2': [
        Case(8, 64, 1, 7, 9, 1, 'one slice of eight channels; a map smaller than an item, odd both ways'),
        Case(24, 64, 1, 17, 33, 1, 'three slices; one row and one column past the items'),
        Case(64, 100, 2, 20, 36, 1, 'two frames, padded channels, ragged items'),
    ],
    'wino2_ws': [
        Case(32, 64, 1, 17, 33, 1, 'one 32-channel chunk; one row and one column past the items'),
        Case(96, 128, 1, 7, 9, 1, 'three chunks, two channel blocks; a map smaller than an item'),
    ],
    'wino4': [
        Case(32, 4, 3, 5, 6, 1, 'one K slice, four output channels of a 128-channel N tile; 2 x 2 tiles per frame, ragged both ways'),
        Case(128, 260, 2, 13, 18, 1, '40 tiles, no multiple of the 128-row GEMM tile; three N tiles, the last with four channels'),
    ],
    'wino4_fused': [
        Case(8, 64, 1, 16, 16, 1, 'one slice; exactly one 16 x 16 item, half a 16 x 32 item'),
        Case(24, 128, 1, 7, 9, 1, 'three slices; a map smaller than an item, no multiple of 4 either way'),
        Case(64, 100, 2, 17, 33, 1, 'ragged in both directions for both item sizes; padded channels'),
        Case(16, 132, 2, 37, 50, 1, 'three item rows; cout_pad 192: the 128-channel form of k_wino4c does not apply'),
        Case(384, 64, 1, 16, 32, 1, '48 slices, the longest ring'),
    ],
    'bf16x3_s1': [
        Case(16, 64, 1, 17, 23, 1, 'one slice; ragged 16 x 16 items'),
        Case(64, 100, 1, 33, 9, 1, 'four slices; padded channels; narrower than an item'),
        Case(16, 512, 2, 33, 250, 1, '512 workgroups of 32 x 16 pixels: the double-buffered 32-row form, its last row tile one pixel high'),
    ],
    'bf16x3_s2': [
        Case(16, 64, 1, 17, 23, 2, 'one slice; odd map'),
        Case(64, 100, 1, 33, 9, 2, 'four slices; padded channels'),
    ],
}

# kernel -> (table, arithmetic 'direct' | 'f2' | 'f4' | 'bf16x3', pack function of pcp_amd.pack, wrapper of pcp_amd.ops, library option or None)
Kernel = namedtuple('Kernel', 'table algo pack op option')
KERNELS = {
    'direct_s1': Kernel('direct_s1', 'direct', 'pack_conv3x3', 'conv3x3', None),
    'direct_s2_form1': Kernel('direct_s2', 'direct', 'pack_conv3x3', 'conv3x3', ('conv_s2_form', 1)),
    'direct_s2_form2': Kernel('direct_s2', 'direct', 'pack_conv3x3', 'conv3x3', ('conv_s2_form', 2)),
    'winograd': Kernel('wino2', 'f2', 'pack_conv3x3_winograd', 'conv3x3_winograd', None),
    'winograd_ws': Kernel('wino2_ws', 'f2', 'pack_conv3x3_winograd_ws', 'conv3x3_winograd_ws', None),
    'winograd4': Kernel('wino4', 'f4', 'pack_conv3x3_winograd4', 'conv3x3_winograd4', None),
    'winograd4f': Kernel('wino4_fused', 'f4', 'pack_conv3x3_winograd4f', 'conv3x3_winograd4f', None),
    'winograd4h': Kernel('wino4_fused', 'f4', 'pack_conv3x3_winograd4h', 'conv3x3_winograd4h', None),
    'winograd4c_nw4': Kernel('wino4_fused', 'f4', 'pack_conv3x3_winograd4c', 'conv3x3_winograd4c', ('wino4c_nw', 4)),
    'winograd4c_nw8': Kernel('wino4_fused', 'f4', 'pack_conv3x3_winograd4c', 'conv3x3_winograd4c', ('wino4c_nw', 8)),
    'bf16x3_s1': Kernel('bf16x3_s1', 'bf16x3', 'pack_conv3x3_bf16x3', 'conv3x3_bf16x3', None),
    'bf16x3_s2': Kernel('bf16x3_s2', 'bf16x3', 'pack_conv3x3_bf16x3', 'conv3x3_bf16x3', None),
}
TABLE_ALGO = {k.table: k.algo for k in KERNELS.values()}
KERNEL_CASES = [(name, i) for name, k in KERNELS.items() for i in range(len(TABLES[k.table]))]
WINO_CASES = [(t, i) for t, a in TABLE_ALGO.items() if a in ('f2', 'f4') for i in range(len(TABLES[t]))]

# the channel-window case of every kernel (index into its table): a ragged one with several slices
WINDOW_CASE = {'direct_s1': 14, 'direct_s2_form1': 14, 'direct_s2_form2': 15, 'winograd': 2, 'winograd_ws': 0, 'winograd4': 1,
               'winograd4f': 2, 'winograd4h': 2, 'winograd4c_nw4': 2, 'winograd4c_nw8': 2, 'bf16x3_s1': 1, 'bf16x3_s2': 1}
PAD_IN, OFF_IN, PAD_OUT, OFF_OUT, FILL = 16, 8, 24, 8, 7.0       # ld_in = cin + 16 read from channel 8, ld_out = cout + 24 written at 8


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case_data(table, i, variant):
    """inputs (float32) and the reference of TABLES[table][i], computed once and read-only.  variant 'ints' | 'float'.  pre is the value
    before the ReLU (the reference with ReLU is np.maximum(pre, 0)), bar the element-wise tolerance of the float variant (None for 'ints')"""
    c = TABLES[table][i]
    algo = TABLE_ALGO[table]
    seed = 6000 + 100 * sorted(TABLES).index(table) + 2 * i + (1 if variant == 'float' else 0)
    shape_x, shape_w = (c.B, c.H, c.W, c.cin), (c.cout, c.cin, 3, 3)
    if variant == 'float':
        x, w, b = uniform(seed, 1, shape_x), uniform(seed, 2, shape_w, -0.05, 0.05), uniform(seed, 3, (c.cout,), -0.2, 0.2)
    elif algo in ('f2', 'f4'):
        x, w, b = wino_int_inputs(seed, shape_x, shape_w)
    else:
        x, w = ints8(seed, 1, shape_x), ints8(seed, 3, shape_w)
        b = np.round(uniform(seed, 5, (c.cout,), -8.0, 8.0)).astype(np.float32)
    pre, S = conv3x3(x, w, b, c.stride, False)
    out = dict(x=x, w=w, b=b, pre=pre, S=S, T=None, bar=None)
    if algo in ('f2', 'f4'):
        out['T'] = wino_scale(x, w, b, 2 if algo == 'f2' else 4)
    if variant == 'float':
        if algo in ('f2', 'f4'):
            out['bar'] = bound(out['T'], c.cin + WINO_ROUNDINGS)
        else:
            out['bar'] = bound(S, 9 * c.cin + 1)
            if algo == 'bf16x3':
                out['bar'] = out['bar'] + B3_RESIDUAL * (S - np.abs(f64(b)))
    return _frozen(out)
