"""Recorder of the output BITS of the CenterHead training kernels, both families of csrc/loss.hip: tests/golden/centerhead_train_bits.json.

pcp_centerhead_targets / pcp_centerhead_loss (one 8-code head) and pcp_centerhead_targets_ext / pcp_centerhead_loss_ext (several heads,
velocity and IoU codes) run one statement of the target assignment, the focal terms and their gradient, the per-head loss and the L1
gradient term.  Their other tests compare each family with a float64 reference inside a derived bound; this file pins every output buffer
to the SHA-256 of its bytes at the commit the JSON names, so the two families cannot drift apart unseen and a change that claims "same
code" is held to it.  tests/test_gpu_centerhead_train_bits.py runs `record()` again and demands equality with the committed file.  Every
launch runs TWICE and the two hashes must agree.

Inputs are seeded and exact to write down (integers times a power of two); `targets_case()` and the `loss_*_case()` generators assert on
the CPU every condition their docstrings name.  What is NOT pinned: losses[0..2] of the many-block one-head case, whose float64 atomics
add block partials in an order that is not fixed (tests/test_gpu_loss.py holds them to their bound).

Record with the library of the commit whose bits are to be pinned (PCP_HIP_LIB selects a library built elsewhere):
    PCP_HIP_LIB=<parent build>/libpcp_hip.so python tests/golden/make_centerhead_train_bits.py --commit <hash of that commit>
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
TABLE = os.path.join(HERE, 'centerhead_train_bits.json')

# ---- targets ----------------------------------------------------------------------------------------------------------------------------
# 20 x 12 cells of 1 m (voxel 0.5, stride 2) from (-10, -6); every coordinate is a multiple of 1 / 16, so the cell arithmetic is exact
TB, TH, TW, TK, TM = 2, 12, 20, 6, 300
STRIDE, VOXEL, MIN_X, MIN_Y, OVERLAP, MIN_RADIUS = 2.0, 0.5, -10.0, -6.0, 0.1, 2
TGT_VARIANTS = {                 # name -> (class sets of the heads, box width, with_iou)
    'one': ([(1, 2, 3)], 8, False),
    'ext10iou': ([(1, 3), (2, 4)], 10, True),
    'ext8': ([(1, 3), (2, 4)], 8, False),
}
# frame -> {row: (class, x, y, dx, dy)}: the foreground rows; z, dz, heading (and vx, vy) are seeded
_FG = {
    0: {3: (1, 5.3125, 2.25, 4.0, 2.0),          # shares cell (15, 8) with row 41
        10: (2, -3.5, 1.5, 0.0, 2.0),            # dx = 0: takes a slot and leaves it empty
        17: (1, 14.0, -2.5, 3.0, 1.5),           # x beyond the range: clamped to W - 0.5
        40: (2, 2.0, -9.0, 2.0, 2.5),            # y below the range: clamped to 0
        41: (3, 5.625, 2.4375, 1.0, 1.0),
        77: (4, -9.5, -5.5, 8.0, 6.0),           # radius past the left and top edges
        100: (3, 9.25, 5.125, 6.0, 5.0),         # radius past the right and bottom edges
        130: (2, 0.5, 0.5, 2.0, 1.0), 131: (1, -4.5, 3.5, 1.5, 3.0), 200: (3, 3.5, -3.5, 2.5, 2.5), 257: (1, -7.5, 0.5, 1.0, 2.0),
        258: (2, 7.5, -4.5, 3.0, 1.0), 280: (4, -1.5, 4.5, 2.0, 2.0), 290: (2, 6.5, 0.5, 1.0, 1.0), 299: (4, -6.5, -2.5, 1.0, 1.0)},
    1: {5: (1, -2.5, -1.5, 3.0, 2.0), 100: (2, 4.5, 3.5, 2.0, 4.0), 260: (3, -8.5, 4.5, 1.5, 1.5), 270: (4, 8.5, -3.5, 2.5, 1.0),
        299: (1, 1.5, 1.5, 5.0, 2.0)},
}


def _radius(height, width, overlap):
    """centernet_utils.py:8-35 in float32, for the generator's own assertions"""
    f = np.float32
    height, width, overlap = f(height), f(width), f(overlap)
    b1 = height + width
    c1 = width * height * ((f(1) - overlap) / (f(1) + overlap))
    r1 = (b1 + np.sqrt(b1 * b1 - f(4) * c1)) / f(2)
    b2 = f(2) * (height + width)
    c2 = (f(1) - overlap) * width * height
    r2 = (b2 + np.sqrt(b2 * b2 - f(16) * c2)) / f(2)
    a3 = f(4) * overlap
    b3 = f(-2) * overlap * (height + width)
    c3 = (overlap - f(1)) * width * height
    r3 = (b3 + np.sqrt(b3 * b3 - f(4) * a3 * c3)) / f(2)
    return min(r1, r2, r3)


def targets_case():
    """gt_boxes (B, 300, 10) float32 [x, y, z, dx, dy, dz, heading, vx, vy, class] (the 8-column form drops vx, vy).  Asserted here, for
    every variant: 300 rows, so the 256-wide ranking loop makes a second trip and rows of it take slots; frame 0 holds more than K rows
    of every head (slots truncate), frame 1 fewer; rows of class 0 and of class 5, which no head owns; and among the rows that take a slot:
    one with dx = 0, one clamped on each axis, two in one cell, one whose radius reaches past the map edge."""
    rs = np.random.RandomState(20240611)
    gt = np.zeros((TB, TM, 10), np.float32)
    for b in range(TB):
        for i in range(TM):
            if i in _FG[b]:
                c, x, y, dx, dy = _FG[b][i]
            elif i % 3 == 0:
                continue                                     # a padding row: all zeros, class 0
            else:
                c, x, y = 5, rs.randint(-160, 160) / 16.0, rs.randint(-96, 96) / 16.0
                dx, dy = rs.randint(8, 80) / 16.0, rs.randint(8, 80) / 16.0
            gt[b, i] = [x, y, rs.randint(-32, 32) / 16.0, dx, dy, rs.randint(16, 48) / 16.0, rs.randint(-50, 50) / 16.0,
                        rs.randint(-64, 64) / 16.0, rs.randint(-64, 64) / 16.0, c]
    assert TM > 256 and (gt[..., 9] == 0).any() and (gt[..., 9] == 5).any()
    for name, (heads, _bw, _iou) in TGT_VARIANTS.items():
        seen = set()
        assert not any(5 in h or 0 in h for h in heads)
        for h in heads:
            rows = [[i for i in range(TM) if gt[b, i, 9] in h] for b in range(TB)]
            assert len(rows[0]) > TK and 0 < len(rows[1]) < TK, (name, h)
            for b in range(TB):
                slots = rows[b][:TK]
                if max(slots) >= 256:
                    seen.add('second trip')
                cells = []
                for i in slots:
                    x, y, dx, dy = gt[b, i, 0], gt[b, i, 1], gt[b, i, 3], gt[b, i, 4]
                    if dx == 0:
                        seen.add('dx = 0')
                        continue
                    cx, cy = (x - MIN_X) / VOXEL / STRIDE, (y - MIN_Y) / VOXEL / STRIDE
                    if cx < 0 or cx > TW - 0.5:
                        seen.add('x clamped')
                    if cy < 0 or cy > TH - 0.5:
                        seen.add('y clamped')
                    ix, iy = int(min(max(cx, 0), TW - 0.5)), int(min(max(cy, 0), TH - 0.5))
                    r = max(int(_radius(dx / VOXEL / STRIDE, dy / VOXEL / STRIDE, OVERLAP)), MIN_RADIUS)
                    if r > min(ix, iy, TW - 1 - ix, TH - 1 - iy) + 1:
                        seen.add('past the edge')
                    cells.append((ix, iy))
                if len(set(cells)) < len(cells):
                    seen.add('shared cell')
        assert seen == {'second trip', 'dx = 0', 'x clamped', 'y clamped', 'past the edge', 'shared cell'}, (name, seen)
    return gt


def _target_heads(variant, d):
    """per head of the variant: dict(num_class, class_to_local and, with the IoU column, a seeded head buffer of pixel stride 16)"""
    class_sets, _bw, with_iou = TGT_VARIANTS[variant]
    heads = []
    for hi, cs in enumerate(class_sets):
        table = [0] * 6
        for local, c in enumerate(cs):
            table[c] = local + 1
        h = dict(num_class=len(cs), class_to_local=table)
        if with_iou:
            g = torch.Generator().manual_seed(300 + hi)
            buf = torch.randint(-16, 17, (TB, TH, TW, 16), generator=g).float() / 16.0       # centre offsets, log dims, rot in [-1, 1]
            h.update(head=buf.to(d), ch_center=0, ch_z=2, ch_dim=3, ch_rot=6)
        heads.append(h)
    return heads


def _targets(got, d):
    from pcp_amd import lib, train_ops as tops
    gt10 = targets_case()
    gt8 = np.ascontiguousarray(gt10[..., [0, 1, 2, 3, 4, 5, 6, 9]])
    names = ('heat', 'target_boxes', 'inds', 'mask')
    for variant, (class_sets, bw, with_iou) in TGT_VARIANTS.items():
        gt = torch.from_numpy(gt10 if bw == 10 else gt8).to(d)
        desc = lib.Target(TB, TH, TW, len(class_sets[0]) if variant == 'one' else 0, TK, STRIDE, VOXEL, VOXEL, MIN_X, MIN_Y, OVERLAP, MIN_RADIUS)
        if variant == 'one':
            got.run('targets|one', lambda: dict(zip(names, tops.centerhead_targets(gt, desc))))
            continue
        heads = _target_heads(variant, d)

        def launch():
            out = tops.centerhead_targets_ext(gt, desc, heads, with_iou=with_iou)
            return {'head %d|%s' % (hi, n): t for hi, per_head in enumerate(out) for n, t in zip(names, per_head)}
        got.run('targets|%s' % variant, launch)


# ---- losses -----------------------------------------------------------------------------------------------------------------------------
LK = 6
CODE_WEIGHTS = [1.0, 1.0, 0.5, 1.0, 0.75, 1.0, 0.25, 1.0, 0.2, 0.2, 1.5]
CLS_WEIGHT, LOC_WEIGHT, GRAD_SCALE = 1.0, 0.25, 0.5


def _loss_head(seed, B, H, W, ncls, n_codes, ld, slots, positives=True, nan_at=None):
    """One head's inputs.  slots: per frame, the (slot, cell) pairs that are masked.  head: integers / 8 in [-5, 5], a few at +-12 where
    the sigmoid clamp is active; heat map: integers / 64 below 1, and 1.0 at each masked cell in a seeded class when `positives`;
    target_boxes: integers / 8, one code of the first masked slot equal to the prediction (its sign term is zero); nan_at = (frame, slot,
    code) plants a NaN target.  Codes are channels 0 .. n_codes - 1, the heat map follows."""
    rs = np.random.RandomState(seed)
    head = rs.randint(-40, 41, (B, H, W, ld)).astype(np.float32) / 8.0
    head.reshape(-1)[rs.choice(head.size, 24, replace=False)] = np.tile([12.0, -12.0], 12)
    heat = rs.randint(0, 61, (B, H, W, ncls)).astype(np.float32) / 64.0
    tb = rs.randint(-40, 41, (B, LK, n_codes)).astype(np.float32) / 8.0
    inds, mask = np.zeros((B, LK), np.int32), np.zeros((B, LK), np.int32)
    for b, frame in enumerate(slots):
        for k, cell in frame:
            inds[b, k], mask[b, k] = cell, 1
            if positives:
                heat[b].reshape(H * W, ncls)[cell, rs.randint(ncls)] = 1.0
        shared = [c for _k, c in frame]
        assert max([shared.count(c) for c in shared] or [0]) <= 2, 'three float atomics onto one cell have no fixed order'
        if frame and b == 0:
            k, cell = frame[0]
            tb[b, k, 1] = head[b].reshape(H * W, ld)[cell, 1]
    if nan_at is not None:
        assert mask[nan_at[0], nan_at[1]]
        tb[nan_at] = np.nan
    assert positives == bool((heat == 1.0).any())
    return dict(head=head, heat=heat, tb=tb, inds=inds, mask=mask, ch_hm=n_codes, num_class=ncls, reg_ch=list(range(n_codes)))


def loss_ext_case():
    """(B, H, W) = (2, 24, 20), K = 6.  Head 0: 3 classes, 8 codes, ld 16 and a gradient buffer of ANOTHER pixel stride (12); slots 1 and 3
    of frame 0 share a cell.  Head 1: 1 class, 11 codes, ld = ld_d = 16, masked slots but no heat-map element equal to 1 in any frame:
    the npos == 0 branch."""
    B, H, W = 2, 24, 20
    h0 = _loss_head(41, B, H, W, 3, 8, 16, [[(0, 17), (1, 203), (2, 479), (3, 203), (4, 0)], [(0, 5), (2, 250), (5, 311)]])
    h1 = _loss_head(42, B, H, W, 1, 11, 16, [[(0, 100), (1, 101)], [(3, 400)]], positives=False)
    h0['ld_d'], h1['ld_d'] = 12, 16
    assert h0['ld_d'] != h0['head'].shape[3] and h1['ld_d'] == h1['head'].shape[3]
    assert list(h0['inds'][0][h0['mask'][0] == 1]).count(203) == 2
    assert h1['mask'].any() and not (h1['heat'] == 1.0).any()
    return (B, H, W), [h0, h1]


def loss_one_cases():
    """name -> ((B, H, W), head, ld_d, pinned losses).  'one block': 256 heat-map elements and 6 slots, so each float64 accumulator
    receives ONE block's sum (onto a zero: exact) and all four losses are pinned; 'one block nan' plants a NaN target in it (the isnotnan
    mask).  'many blocks': 2880 elements = 12 blocks of k_focal_reduce, so only losses[3] (num_pos, a sum of ones: exact in any order) and
    dhead (which reads the integer counts only) are pinned.  In every case at most two masked slots of a frame share a cell: the float
    atomics of k_reg_grad add at most two terms onto a zero, which is order-free."""
    slots_a = [[(0, 9), (1, 77), (3, 9), (5, 127)]]
    cases = {
        'one block': ((1, 8, 16), _loss_head(51, 1, 8, 16, 2, 8, 16, slots_a), 12, slice(0, 4)),
        'one block nan': ((1, 8, 16), _loss_head(51, 1, 8, 16, 2, 8, 16, slots_a, nan_at=(0, 1, 2)), 12, slice(0, 4)),
        'many blocks': ((2, 24, 20), _loss_head(52, 2, 24, 20, 3, 8, 16, [[(0, 17), (1, 203), (2, 479), (4, 203)], [(1, 5), (2, 5), (5, 311)]]),
                        16, slice(3, 4)),
    }
    for name, ((B, H, W), h, _ld_d, pinned) in cases.items():
        blocks = (B * H * W * h['num_class'] + 255) // 256
        assert B * LK <= 256                                      # one block of k_reg_reduce: the mask sum and the L1 sums are one block's
        assert (blocks == 1) == (pinned == slice(0, 4)), name
    assert np.isnan(cases['one block nan'][1]['tb']).sum() == 1 and not np.isnan(cases['one block'][1]['tb']).any()
    return cases


def _dev(a, d):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def _losses(got, d):
    from pcp_amd import lib, train_ops as tops
    (B, H, W), heads = loss_ext_case()
    desc = lib.HeadLossExt()
    desc.batch, desc.h, desc.w, desc.k = B, H, W, LK
    desc.cls_weight, desc.loc_weight = CLS_WEIGHT, LOC_WEIGHT
    for j, v in enumerate(CODE_WEIGHTS):
        desc.code_weights[j] = v
    on_dev = [{k: (_dev(v, d) if isinstance(v, np.ndarray) else v) for k, v in h.items()} for h in heads]
    for with_grad in (True, False):
        def launch():
            args = [dict(h, dhead=torch.full((B, H, W, h['ld_d']), -7.0, device=d)) for h in on_dev]
            losses, total, dheads = tops.centerhead_loss_ext(desc, args, with_grad=with_grad, grad_scale=GRAD_SCALE)
            out = {'losses': losses, 'total': total}
            if with_grad:
                out.update({'dhead %d' % i: g for i, g in enumerate(dheads)})
            return out
        got.run('loss_ext|%s' % ('grad' if with_grad else 'no grad'), launch)

    for name, ((B, H, W), h, ld_d, pinned) in loss_one_cases().items():
        d1 = lib.HeadLoss()
        d1.batch, d1.h, d1.w, d1.ld, d1.ld_d, d1.num_class, d1.ch_hm, d1.k = B, H, W, h['head'].shape[3], ld_d, h['num_class'], h['ch_hm'], LK
        for j in range(8):
            d1.reg_ch[j], d1.code_weights[j] = h['reg_ch'][j], CODE_WEIGHTS[j]
        d1.cls_weight, d1.loc_weight = CLS_WEIGHT, LOC_WEIGHT
        t = {k: _dev(h[k], d) for k in ('head', 'heat', 'tb', 'inds', 'mask')}

        def launch():
            dhead = torch.full((B, H, W, ld_d), -7.0, device=d)
            losses = tops.centerhead_loss(t['head'], d1, t['heat'], t['tb'], t['inds'], t['mask'], dhead=dhead, grad_scale=GRAD_SCALE)
            return {'losses[%d:%d]' % (pinned.start, pinned.stop): losses[pinned], 'dhead': dhead}
        got.run('loss_one|%s' % name, launch)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


class _Table(dict):
    def run(self, key, launch):
        """launch() -> {buffer name: tensor}; run twice, the hashes of the two runs must agree"""
        first, second = ({n: _sha(t) for n, t in launch().items()} for _ in range(2))
        assert first == second, '%s: two runs of one launch gave different bits' % key
        for n, h in first.items():
            assert key + '|' + n not in self, key
            self[key + '|' + n] = h


def record():
    """key -> SHA-256 of the buffer's bytes"""
    d = torch.device('cuda:0')
    got = _Table()
    _targets(got, d)
    _losses(got, d)
    torch.cuda.synchronize()
    return dict(got)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the loaded library was built from')
    ap.add_argument('--out', default=TABLE)
    args = ap.parse_args()
    from pcp_amd import lib
    doc = {'recorded_at_commit': args.commit, 'sha256': record()}
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%s: %d buffers of the library %s, recorded at %s' % (args.out, len(doc['sha256']), lib.LIB_PATH, args.commit))
