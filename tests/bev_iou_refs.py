"""Float64 references and seeded case builders for the rotated BEV IoU / NMS kernels of csrc/nms.hip (tests/test_bev_iou_refs_cpu.py,
tests/test_gpu_bev_iou.py).  numpy only.

The geometry here is independent of oracle/nms_oracle.c and csrc/bev_geom.h on purpose: those two restate the same reference arithmetic
(edge crossings + corner-in tests with a 1e-2 margin + an atan2 sort of the vertices); this file clips one rectangle by the four half
planes of the other (Sutherland-Hodgman) in float64 and takes the shoelace area of what is left.  No margin, no EPS.

Boxes are rows (x, y, z, dx, dy, dz, heading); only x, y, dx, dy, heading matter.  The float32 input values are taken as exact.
"""
import numpy as np

NMS_MARGIN = 1e-2                      # csrc/bev_geom.h: a corner counts as inside up to this far outside
GENERIC_CLEARANCE = 2 * NMS_MARGIN     # a pair is generic when no corner is this close to the other box's boundary


# ---- float64 geometry ------------------------------------------------------------------------------------------------------------------

def _f64(boxes):
    b = np.asarray(boxes, dtype=np.float64)
    return b.reshape(-1, b.shape[-1])


def _corners_about(boxes, ox, oy):
    """corners of boxes (P, 7), counter-clockwise, relative to the origin (ox, oy) (P,): (P, 4, 2).  Subtracting the origin first is exact for
    float32 inputs and keeps the products small at |x|, |y| ~ 100 m."""
    hx, hy = boxes[:, 3] / 2, boxes[:, 4] / 2
    c, s = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    lx = np.stack([-hx, hx, hx, -hx], 1)
    ly = np.stack([-hy, -hy, hy, hy], 1)
    x = lx * c[:, None] - ly * s[:, None] + (boxes[:, 0] - ox)[:, None]
    y = lx * s[:, None] + ly * c[:, None] + (boxes[:, 1] - oy)[:, None]
    return np.stack([x, y], 2)


def corners64(boxes):
    """(n, 7) -> (n, 4, 2) float64 world corners, counter-clockwise from the (-dx/2, -dy/2) corner"""
    b = _f64(boxes)
    return _corners_about(b, np.zeros(b.shape[0]), np.zeros(b.shape[0]))


def _clip_halfplane(poly, cnt, p0, p1):
    """one Sutherland-Hodgman step for P polygons at once: poly (P, M, 2) with cnt (P,) valid vertices, kept on the left of p0 -> p1 (P, 2)."""
    P, M, _ = poly.shape
    idx = np.arange(M)[None, :]
    valid = idx < cnt[:, None]
    nxt_i = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    nxt = np.take_along_axis(poly, nxt_i[:, :, None], axis=1)
    e = (p1 - p0)[:, None, :]
    d_cur = e[..., 0] * (poly[..., 1] - p0[:, None, 1]) - e[..., 1] * (poly[..., 0] - p0[:, None, 0])
    d_nxt = e[..., 0] * (nxt[..., 1] - p0[:, None, 1]) - e[..., 1] * (nxt[..., 0] - p0[:, None, 0])
    in_cur, in_nxt = d_cur >= 0, d_nxt >= 0
    cross = valid & (in_cur != in_nxt)
    den = np.where(cross, d_cur - d_nxt, 1.0)
    t = d_cur / den
    inter = poly + t[..., None] * (nxt - poly)
    cand = np.stack([poly, inter], 2).reshape(P, 2 * M, 2)                 # vertex i, then the crossing on edge i -> i + 1
    mask = np.stack([valid & in_cur, cross], 2).reshape(P, 2 * M)
    order = np.argsort(~mask, axis=1, kind='stable')                       # emitted points first, in their order
    out = np.take_along_axis(cand, order[:, :, None], axis=1)[:, :M]
    n_out = mask.sum(1)
    assert n_out.max(initial=0) <= M
    return np.where((np.arange(M)[None, :] < n_out[:, None])[..., None], out, 0.0), n_out


def _overlap_rows(a, b):
    """area of a[k] ∩ b[k], (P,)"""
    P = a.shape[0]
    if P == 0:
        return np.zeros(0)
    ox, oy = a[:, 0], a[:, 1]
    ca, cb = _corners_about(a, ox, oy), _corners_about(b, ox, oy)
    poly = np.zeros((P, 12, 2))                                             # an octagon at most, plus room for doubled vertices on coincident edges
    poly[:, :4] = ca
    cnt = np.full(P, 4)
    for k in range(4):
        poly, cnt = _clip_halfplane(poly, cnt, cb[:, k], cb[:, (k + 1) % 4])
    idx = np.arange(12)[None, :]
    nxt_i = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    nxt = np.take_along_axis(poly, nxt_i[:, :, None], axis=1)
    v, w = poly - poly[:, :1], nxt - poly[:, :1]                            # shoelace about the first vertex
    tw = np.where(idx < cnt[:, None], v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0], 0.0).sum(1)
    area = np.where(cnt >= 3, np.abs(tw) / 2, 0.0)
    flat = (a[:, 3] * a[:, 4] == 0) | (b[:, 3] * b[:, 4] == 0)              # a box without area has no half planes to clip by
    return np.where(flat, 0.0, area)


def _pairs(a, b, rows):
    a, b = _f64(a), _f64(b)
    if rows:
        assert a.shape[0] == b.shape[0]
        return a, b, (a.shape[0],)
    na, nb = a.shape[0], b.shape[0]
    return np.repeat(a, nb, 0), np.tile(b, (na, 1)), (na, nb)


def overlap64(a, b, rows=False):
    """area of rectangle ∩ rectangle in float64: the (na, nb) matrix, or with rows=True the (n,) areas of a[k] ∩ b[k]"""
    a, b, shape = _pairs(a, b, rows)
    return _overlap_rows(a, b).reshape(shape)


def iou64(a, b, rows=False):
    """ov / (sa + sb - ov) in float64; 0 where the union has no area"""
    a, b, shape = _pairs(a, b, rows)
    ov = _overlap_rows(a, b)
    union = a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - ov
    return np.where(union > 0, ov / np.where(union > 0, union, 1.0), 0.0).reshape(shape)


def _boundary_distance(box, pts):
    """distance of points pts (P, K, 2) to the boundary of box (P, 7), from inside or outside: (P, K)"""
    c, s = np.cos(box[:, 6])[:, None], np.sin(box[:, 6])[:, None]
    px, py = pts[..., 0] - box[:, None, 0], pts[..., 1] - box[:, None, 1]
    u, v = np.abs(px * c + py * s), np.abs(-px * s + py * c)
    ex, ey = u - box[:, None, 3] / 2, v - box[:, None, 4] / 2              # > 0: outside along that axis
    outside = np.hypot(np.maximum(ex, 0), np.maximum(ey, 0))
    inside = np.minimum(-ex, -ey)
    return np.where((ex > 0) | (ey > 0), outside, inside)


def clearance64(a, b, rows=False):
    """the smallest distance from any corner of either box to the other box's boundary; a pair is generic when this is >= GENERIC_CLEARANCE"""
    a, b, shape = _pairs(a, b, rows)
    n = a.shape[0]
    zero = np.zeros(n)
    ca, cb = _corners_about(a, zero, zero), _corners_about(b, zero, zero)
    d = np.minimum(_boundary_distance(a, cb).min(1), _boundary_distance(b, ca).min(1)) if n else zero
    return d.reshape(shape)


def near_pairs(a, b):
    """(na, nb) bool: centre distance below the sum of the half diagonals (the boxes can touch at all)"""
    a, b = _f64(a), _f64(b)
    ra, rb = np.hypot(a[:, 3], a[:, 4]) / 2, np.hypot(b[:, 3], b[:, 4]) / 2
    return np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]) < ra[:, None] + rb[None, :]


# ---- the sweep and the sort ------------------------------------------------------------------------------------------------------------

def greedy_nms(hit_matrix, post_max=None):
    """greedy suppression on a boolean (n, n) matrix whose rows / columns are in score order: row i, if alive, is kept and kills every later j
    with hit[i, j].  Stops after post_max kept rows.  -> int64 indices"""
    hit = np.asarray(hit_matrix, dtype=bool)
    n = hit.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if post_max is not None and len(keep) >= post_max:
            break
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= hit[i, i + 1:]
    return np.asarray(keep, dtype=np.int64)


def stable_desc_order(scores):
    """the reference's order: descending, equal scores in index order; -0.0 == +0.0 under it"""
    return np.argsort(-np.asarray(scores), kind='stable')


# ---- seeded case builders --------------------------------------------------------------------------------------------------------------

def _box_rows(n):
    b = np.zeros((n, 7), np.float32)
    b[:, 5] = 1.5
    return b


def clustered(seed, n):
    """n boxes jittered +-2 m around 20 centres in +-40 m, 0.5-6 m x 0.4-2.5 m, headings in +-3.3 rad: dense in overlapping pairs"""
    rng = np.random.RandomState(seed)
    ctr = rng.uniform(-40, 40, (20, 2))
    which = rng.randint(0, 20, n)
    b = _box_rows(n)
    b[:, 0:2] = ctr[which] + rng.uniform(-2, 2, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3] = rng.uniform(0.5, 6.0, n)
    b[:, 4] = rng.uniform(0.4, 2.5, n)
    b[:, 6] = rng.uniform(-3.3, 3.3, n)
    return b


DEGENERATE_CENTRES = ((0.0, 0.0), (48.3, -37.7), (-100.4, 99.9))
DEGENERATE_HEADINGS = (0.0, 1e-4, 0.3, np.pi / 4, np.pi / 2, 3.0, np.pi, -np.pi)


def degenerate_table():
    """-> (a (m, 7), b (m, 7), exact_iou (m,), exact_overlap (m,), kind list): pairs whose IoU has a closed form, at every centre and heading of
    DEGENERATE_CENTRES x DEGENERATE_HEADINGS (1.6 / 7.98 for the concentric pair, 1/16, 1/3, 1/7, ...).  The closed forms use the float32 values
    of the sizes; the float32 rounding of centre + shift (8e-6 m at 100 m) moves an overlap by < 2e-5 m^2 and an IoU by < 1e-6."""
    A, Bx, iou, ov, kind = [], [], [], [], []

    def row(k, a, b, i, o):
        A.append(a), Bx.append(b), iou.append(i), ov.append(o), kind.append(k)

    def box(cx, cy, dx, dy, ang):
        return [cx, cy, 0.0, dx, dy, 1.5, ang]

    for cx, cy in DEGENERATE_CENTRES:
        for ang in DEGENERATE_HEADINGS:
            ux, uy = np.cos(ang), np.sin(ang)
            L, W = float(np.float32(4.2)), float(np.float32(1.9))
            S = float(np.float32(0.8))
            row('identical', box(cx, cy, L, W, ang), box(cx, cy, L, W, ang), 1.0, L * W)
            row('plus_pi', box(cx, cy, L, W, ang), box(cx, cy, L, W, ang + np.pi), 1.0, L * W)
            row('concentric', box(cx, cy, 2.0, S, ang), box(cx, cy, L, W, ang), 2.0 * S / (L * W), 2.0 * S)
            row('turned_inside', box(cx, cy, 1.0, 1.0, ang + 0.5), box(cx, cy, 4.0, 4.0, ang), 1.0 / 16, 1.0)
            row('shared_edge', box(cx, cy, 4.0, 2.0, ang), box(cx + 4.0 * ux, cy + 4.0 * uy, 4.0, 2.0, ang), 0.0, 0.0)
            row('half_shift', box(cx, cy, 4.0, 2.0, ang), box(cx + 2.0 * ux, cy + 2.0 * uy, 4.0, 2.0, ang), 1.0 / 3, 4.0)
            row('crossed', box(cx, cy, 4.0, 1.0, ang), box(cx, cy, 4.0, 1.0, ang + np.pi / 2), 1.0 / 7, 1.0)
            row('far', box(cx, cy, L, W, ang), box(cx + 30.0, cy - 20.0, L, W, ang + 0.7), 0.0, 0.0)
            row('zero_zero', box(cx, cy, 0.0, 0.0, ang), box(cx, cy, 0.0, 0.0, ang), 0.0, 0.0)
            row('zero_in_2x2', box(cx, cy, 0.0, 0.0, ang), box(cx, cy, 2.0, 2.0, ang), 0.0, 0.0)
    f = np.float32
    return np.asarray(A, f), np.asarray(Bx, f), np.asarray(iou), np.asarray(ov), kind


def tiny_pairs():
    """boxes of the size of NMS_MARGIN: 0.05 m squares, the second shifted by 0.005 m along x or along the diagonal, at each centre of the table.
    True IoU 9/11 and 81/119; the reference arithmetic takes all eight corners as inside the other square (each is within the 1e-2 margin),
    fans over their hull and returns an IoU above 1."""
    a = np.asarray([[cx, cy, 0.0, 0.05, 0.05, 1.5, 0.0] for cx, cy in DEGENERATE_CENTRES for _k in range(2)], np.float32)
    b = a.copy()
    b[:, 0] += np.float32(0.005)
    b[1::2, 1] += np.float32(0.005)
    return a, b


def far_apart_grid(n, seed=0, pitch=10.0):
    """n boxes on a square grid of the given pitch, up to 5.5 m x 2.5 m with seeded headings: no two overlap, whatever the order"""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(max(n, 1))))
    k = np.arange(n)
    b = _box_rows(n)
    b[:, 0] = (k % side - side / 2) * pitch
    b[:, 1] = (k // side - side / 2) * pitch
    b[:, 3] = rng.uniform(3.0, 5.5, n)
    b[:, 4] = rng.uniform(1.5, 2.5, n)
    b[:, 6] = rng.uniform(-3.14, 3.14, n)
    return b


CHAIN_LENGTH, CHAIN_WIDTH, CHAIN_PITCH = 4.0, 2.0, 2.25


def chain_line(n, x0=0.0, y0=0.0):
    """-> (boxes, hit): n equal axis-aligned 4 x 2 boxes on a line along x, 2.25 m apart.  Neighbours overlap with IoU 1.75 / 6.25 = 0.28,
    second neighbours are 0.5 m apart and do not overlap: hit[i, j] = |i - j| == 1 for any threshold in (0.01, 0.27).  Every coordinate is a
    multiple of 0.25 below 2^14, exact in float32.  In line order the greedy sweep keeps every other box: 0, 2, 4, ..."""
    b = _box_rows(n)
    b[:, 0] = x0 + CHAIN_PITCH * np.arange(n)
    b[:, 1] = y0
    b[:, 3], b[:, 4] = CHAIN_LENGTH, CHAIN_WIDTH
    i = np.arange(n)
    return b, np.abs(i[:, None] - i[None, :]) == 1


def duplicates_across_blocks():
    """-> (boxes (266, 7) in score order, keep): far-apart distinct boxes; the box at row 5 has exact copies at rows 40, 64, 127, 133, 255 and 265,
    that is in its own 64-row block and in every later one, on first, last and inner rows.  Every copy is suppressed (IoU 1) by row 5 and
    nothing else is: keep is every row but the copies."""
    n = 266
    copies = [40, 64, 127, 133, 255, 265]
    b = far_apart_grid(n, seed=7)
    b[copies] = b[5]
    return b, np.setdiff1d(np.arange(n), copies)


def three_block_chain():
    """-> (boxes (192, 7) in score order, keep): far-apart boxes on a grid around the origin, and three chain_line boxes A (row 10, block 0),
    B (row 84, block 1), C (row 158, block 2) on a line at y = 500: A-B and B-C overlap with IoU 0.28, A-C do not touch.  A suppresses B; B,
    being suppressed, must not suppress C: keep is every row but 84."""
    n = 192
    b = far_apart_grid(n, seed=11)
    chain, _hit = chain_line(3, x0=0.0, y0=500.0)
    b[[10, 84, 158]] = chain
    return b, np.setdiff1d(np.arange(n), [84])


def threshold_safe(boxes, thr, gap, iou_fn=None):
    """drop boxes, deterministically (pairs in row-major order, the later box of a pair goes), until no pair's IoU under iou_fn -- the oracle's
    float32 rotated IoU by default -- lies within gap of thr; -> the survivors, in order.  Any subset of the result is safe too."""
    if iou_fn is None:
        from oracle import nms as onms
        iou_fn = onms.iou_matrix
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    iou = iou_fn(boxes, boxes).astype(np.float64)
    bad = np.abs(iou - thr) < gap
    bad = np.triu(bad | bad.T, 1)
    alive = np.ones(boxes.shape[0], bool)
    for i, j in np.argwhere(bad):
        if alive[i] and alive[j]:
            alive[j] = False
    return boxes[alive]
