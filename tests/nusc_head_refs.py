"""Plain float64 numpy statements of the multi-head CenterHead training arithmetic (target assignment with per-head class tables and
velocity columns, the IoU target, focal + L1 losses), written from the reference's semantics (pcdet/models/dense_heads/center_head.py:105-300,
dense_heads/box_utils.py:6-67, model_utils/centernet_utils.py:8-68, utils/loss_utils.py:264-343).  tests/test_nusc_head_train_cpu.py shows
that they reproduce what the reference's own CenterHead produced (fixture g21); the GPU tests then use them for cases the fixture lacks."""
import numpy as np


def class_tables(class_names, class_names_each_head):
    """per head: table[global class id] = 1-based index inside the head, 0 = not in the head ([0] = padding rows)"""
    out = []
    for names in class_names_each_head:
        t = [0] * (len(class_names) + 1)
        for local, n in enumerate(names):
            t[class_names.index(n) + 1] = local + 1
        out.append(t)
    return out


def gaussian_radius(h, w, ov):
    b1 = h + w
    c1 = w * h * (1 - ov) / (1 + ov)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (h + w)
    c2 = (1 - ov) * w * h
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * ov
    b3 = -2 * ov * (h + w)
    c3 = (ov - 1) * w * h
    r3 = (b3 + np.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def aa_rect(x, y, dx, dy, angle):
    """box_utils.py:6-25: the sign table [[1,1,-1,-1],[-1,1,1,-1],[1,1,1,1]] is .view(4, 3)-ed, not transposed: the rows become
    (1,1,-1), (-1,-1,1), (1,-1,1), (1,1,1), i.e. the xy corners (+,+), (-,-), (+,-), (+,+)"""
    c, s = np.cos(angle), np.sin(angle)
    xs, ys = [], []
    for sx, sy in ((1, 1), (-1, -1), (1, -1), (1, 1)):
        lx, ly = 0.5 * dx * sx, 0.5 * dy * sy
        xs.append(lx * c - ly * s + x)
        ys.append(lx * s + ly * c + y)
    return min(xs), min(ys), max(xs), max(ys)


def aa_iou(a, b):
    inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    a1 = max(a[2] - a[0], 0.0) * max(a[3] - a[1], 0.0)
    a2 = max(b[2] - b[0], 0.0) * max(b[3] - b[1], 0.0)
    u = a1 + a2 - inter
    return inter / u if u > 0 else 0.0


def assign_targets(gt, tables, geom, K, heads=None):
    """gt (B, M, 8 | 10).  tables: class_tables().  geom: dict(h, w, stride, voxel_x, voxel_y, min_x, min_y, overlap, min_radius).
    heads: None, or per head dict(maps (B, H, W, C) NHWC raw head maps, center, center_z, dim, rot channel offsets) -> the IoU column.
    Returns per head dict(heat (B, H, W, ncls), tb (B, K, T), inds (B, K), mask (B, K), radius [(b, slot, float radius)])."""
    gt = np.asarray(gt, dtype=np.float64)
    B, M, bw = gt.shape
    tw = 8 + (2 if bw == 10 else 0) + (1 if heads is not None else 0)
    H, W = geom['h'], geom['w']
    out = []
    for hi, table in enumerate(tables):
        ncls = max(table)
        heat = np.zeros((B, H, W, ncls))
        tb = np.zeros((B, K, tw))
        inds = np.zeros((B, K), dtype=np.int64)
        mask = np.zeros((B, K), dtype=np.int64)
        radii = []
        for b in range(B):
            k = -1
            for i in range(M):
                r = gt[b, i]
                gc = int(r[-1])
                local = table[gc] if 0 <= gc < len(table) else 0
                if local == 0:
                    continue
                k += 1
                if k >= K:
                    break
                cx = (r[0] - geom['min_x']) / geom['voxel_x'] / geom['stride']
                cy = (r[1] - geom['min_y']) / geom['voxel_y'] / geom['stride']
                cx = min(max(cx, 0.0), W - 0.5)
                cy = min(max(cy, 0.0), H - 0.5)
                ix, iy = int(cx), int(cy)
                dx = r[3] / geom['voxel_x'] / geom['stride']
                dy = r[4] / geom['voxel_y'] / geom['stride']
                if dx <= 0 or dy <= 0:
                    continue
                rad = gaussian_radius(dx, dy, geom['overlap'])
                radii.append((b, k, rad))
                ri = max(int(rad), geom['min_radius'])
                inds[b, k] = iy * W + ix
                mask[b, k] = 1
                tb[b, k, :8] = [cx - ix, cy - iy, r[2], np.log(r[3]), np.log(r[4]), np.log(r[5]), np.cos(r[6]), np.sin(r[6])]
                if bw == 10:
                    tb[b, k, 8:10] = r[7:9]
                if heads is not None:
                    hd = heads[hi]
                    px = np.asarray(hd['maps'][b, iy, ix], dtype=np.float64)
                    pxw = (ix + px[hd['center']]) * geom['stride'] * geom['voxel_x'] + geom['min_x']
                    pyw = (iy + px[hd['center'] + 1]) * geom['stride'] * geom['voxel_y'] + geom['min_y']
                    ang = np.arctan2(px[hd['rot'] + 1], px[hd['rot']])
                    ra = aa_rect(pxw, pyw, np.exp(px[hd['dim']]), np.exp(px[hd['dim'] + 1]), ang)
                    rb = aa_rect(r[0], r[1], r[3], r[4], r[6])
                    tb[b, k, tw - 1] = 2.0 * aa_iou(ra, rb) - 1.0
                sigma = (2 * ri + 1) / 6.0
                left, right = min(ix, ri), min(W - ix, ri + 1)
                top, bottom = min(iy, ri), min(H - iy, ri + 1)
                ys, xs = np.mgrid[-top:bottom, -left:right]
                gs = np.exp(-(xs * xs + ys * ys) / (2 * sigma * sigma))
                sl = heat[b, iy - top:iy + bottom, ix - left:ix + right, local - 1]
                np.maximum(sl, gs, out=sl)
        out.append(dict(heat=heat, tb=tb, inds=inds, mask=mask, radius=radii))
    return out


def head_loss(maps, ch_hm, ncls, reg_ch, heat, tb, inds, mask, code_weights, cls_weight, loc_weight, heat_is_one=None):
    """one head.  maps (B, H, W, C) raw NHWC; heat (B, H, W, ncls); tb (B, K, T), T == len(reg_ch).  heat_is_one: boolean array marking the
    positives (default heat == 1).  Returns dict(hm, loc, num_pos, dmaps (B, H, W, C) = d(hm + loc)/d maps)."""
    if tb.shape[-1] != len(reg_ch):
        raise ValueError('target_boxes has %d columns but %d prediction channels' % (tb.shape[-1], len(reg_ch)))
    maps = np.asarray(maps, dtype=np.float64)
    heat = np.asarray(heat, dtype=np.float64)
    B, H, W, C = maps.shape
    x = maps[..., ch_hm:ch_hm + ncls]
    s = 1.0 / (1.0 + np.exp(-x))
    inside = (s >= 1e-4) & (s <= 1 - 1e-4)
    p = np.clip(s, 1e-4, 1 - 1e-4)
    pos = (heat == 1) if heat_is_one is None else heat_is_one
    neg = ~pos & (heat < 1)
    nw = (1 - heat) ** 4
    pos_l = np.where(pos, np.log(p) * (1 - p) ** 2, 0.0).sum()
    neg_l = np.where(neg, np.log(1 - p) * p ** 2 * nw, 0.0).sum()
    npos = int(pos.sum())
    hm = (-neg_l if npos == 0 else -(pos_l + neg_l) / npos) * cls_weight
    dldp = np.where(pos, (1 - p) ** 2 / p - 2 * (1 - p) * np.log(p), 0.0) * (0.0 if npos == 0 else 1.0)
    dldp = dldp + np.where(neg, nw * (-(p ** 2) / (1 - p) + 2 * p * np.log(1 - p)), 0.0)
    dmaps = np.zeros_like(maps)
    dmaps[..., ch_hm:ch_hm + ncls] = np.where(inside, -cls_weight / max(npos, 1) * dldp * p * (1 - p), 0.0)
    num = max(float(mask.sum()), 1.0)
    flat = maps.reshape(B, H * W, C)
    dflat = dmaps.reshape(B, H * W, C)
    loc = 0.0
    for j, ch in enumerate(reg_ch):
        tot = 0.0
        for b in range(B):
            for k in np.nonzero(mask[b])[0]:
                diff = flat[b, inds[b, k], ch] - tb[b, k, j]
                tot += abs(diff)
                dflat[b, inds[b, k], ch] += np.sign(diff) * loc_weight * code_weights[j] / num
        loc += tot / num * code_weights[j]
    loc *= loc_weight
    return dict(hm=hm, loc=loc, num_pos=npos, dmaps=dmaps)
