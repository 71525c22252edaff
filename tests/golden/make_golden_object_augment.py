"""Generates tests/golden/g28_object_augment.npz: the reference's OWN per-object augmentation (DataAugmentor.random_local_translation /
_rotation / _scaling, random_local_frustum_dropout, random_world_frustum_dropout through augmentor_utils, the world rotation and flip of
the full list, the final limit_period), run sample by sample on float32 inputs after np.random.seed(s).  Runs only where the reference
is mounted (ref_harness); the fixture holds inputs, every np.random.uniform value in call order and the results, no program text.

Shapes: three frames of 700, 0 and 613 rows (a 512-row tile straddles frames 0 and 2, frame 1 is empty) with 9, 0 and 1 boxes in a padded
M = 12.  Boxes 0 and 1 of frame 0 overlap (rows inside both); boxes 3 and 4 stand end to end along x so that a positive x translation
pushes rows of box 3 into box 4, which moves them again (asserted below for the cases named in meta['order_dependent']).  The last
feature column holds the row's index, which is how the rows are followed through the dropouts.

The reference's global_frustum_dropout_* raise on a sample without points (np.max of an empty array); for the empty frame this generator
makes the entry's np.random.uniform calls itself and leaves the sample alone, which is what the device path defines for it.

Conditioning: the walk is restated in float64 and in float32 (tests/object_augment_refs.py).  margin = 10 x the largest difference between
the float32 and the float64 value of any face or threshold distance, measured here; every row closer than that to a face or threshold at
any box visit is redrawn until none is.  Asserted here: the float64 restatement finds the rows the reference's get_points_in_box found,
at every visit, and keeps the rows and boxes the reference kept.  meta['conditioning'] records margin, the measured difference and the
smallest distance left.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import object_augment_refs as oar  # noqa: E402
import ref_harness  # noqa: E402

OUT = os.path.join(HERE, 'g28_object_augment.npz')
SIZES, N_BOXES, M_PAD = [700, 0, 613], [9, 0, 1], 12
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]

LT = lambda axes: {'NAME': 'random_local_translation', 'LOCAL_TRANSLATION_RANGE': [0.2, 0.9], 'ALONG_AXIS_LIST': axes}  # noqa: E731
LROT = {'NAME': 'random_local_rotation', 'LOCAL_ROT_ANGLE': 0.3}
LROT2 = {'NAME': 'random_local_rotation', 'LOCAL_ROT_ANGLE': [-0.2, 0.4]}
LSC = {'NAME': 'random_local_scaling', 'LOCAL_SCALE_RANGE': [0.8, 1.2]}
LSC0 = {'NAME': 'random_local_scaling', 'LOCAL_SCALE_RANGE': [1.0, 1.0005]}
LDROP = lambda d: {'NAME': 'random_local_frustum_dropout', 'INTENSITY_RANGE': [0.1, 0.4], 'DIRECTION': d}  # noqa: E731
WDROP = lambda d: {'NAME': 'random_world_frustum_dropout', 'INTENSITY_RANGE': [0.05, 0.2], 'DIRECTION': d}  # noqa: E731
WROT = {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.3, 0.3]}
WFLIP = {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}

CASES = [dict(name='lt_%s' % a, C=4, W=8, seed=21 + i, lst=[LT([a])]) for i, a in enumerate('xyz')]
CASES += [dict(name='lrot', C=5, W=8, seed=31, lst=[LROT]), dict(name='lscale', C=5, W=8, seed=32, lst=[LSC]),
          dict(name='lscale_skip', C=5, W=8, seed=33, lst=[LSC0, LROT2])]
CASES += [dict(name='ldrop_%s' % d, C=5, W=8, seed=41 + i, lst=[LDROP([d])]) for i, d in enumerate(oar.DIRECTIONS)]
CASES += [dict(name='wdrop_%s' % d, C=5, W=8, seed=51 + i, lst=[WDROP([d])]) for i, d in enumerate(oar.DIRECTIONS)]
CASES += [dict(name='full', C=12, W=8, seed=61,
               lst=[WROT, LT(['x', 'y', 'z']), LROT, LSC, LDROP(['top', 'left']), WDROP(['bottom', 'right']), WFLIP]),
          dict(name='w10', C=4, W=10, seed=62, lst=[LT(['x', 'y', 'z']), LSC, LDROP(['bottom', 'right']), WDROP(['top', 'left'])])]
ORDER_DEPENDENT = ['lt_x', 'full', 'w10']


def make_boxes(rng, m, W):
    g = np.zeros((m, W), dtype=np.float32)
    grid = [(-36, -30), (-8, -34), (22, -30), (-38, 14), (-6, 26), (20, 30), (38, 0), (-24, 36), (6, -8)]
    for i in range(m):
        g[i, 0:2] = np.asarray(grid[i % len(grid)]) + rng.uniform(-2, 2, 2)
        g[i, 2] = rng.uniform(-2.0, -0.5)
        g[i, 3:6] = [rng.uniform(3.5, 5.0), rng.uniform(1.6, 2.4), rng.uniform(1.4, 2.0)]
        g[i, 6] = rng.uniform(-3.0, 3.0)
    if m >= 5:
        g[1, 0:3] = g[0, 0:3] + np.asarray([1.2, 0.5, 0.1], np.float32)            # box 1 overlaps box 0
        g[3, 6] = g[4, 6] = 0.0                                                   # boxes 3 and 4 end to end along x
        g[4, 0:3] = g[3, 0:3] + np.asarray([(g[3, 3] + g[4, 3]) / 2 + 0.15, 0.0, 0.0], np.float32)
        g[4, 4:6] = g[3, 4:6]
    if W == 10:
        g[:, 7:9] = rng.uniform(-8, 8, (m, 2))
    g[:, W - 1] = rng.integers(1, 4, m)
    return g


def make_rows(rng, n, C, gt, only_background=False):
    p = np.zeros((n, C), dtype=np.float32)
    p[:, 0:2] = rng.uniform(-50.0, 50.0, (n, 2))
    p[:, 2] = rng.uniform(-4.0, 2.0, n)
    k = 0
    per = 0 if only_background or gt.shape[0] == 0 else min(45 if gt.shape[0] > 1 else 60, n // gt.shape[0])
    for box in gt:
        loc = rng.uniform(-0.65, 0.65, (per, 3)) * box[3:6]
        if k // max(per, 1) == 3:
            loc[:, 0] = np.abs(loc[:, 0])                                         # box 3: the +x half, next to box 4
        c, s = np.cos(box[6]), np.sin(box[6])
        p[k:k + per, 0] = box[0] + loc[:, 0] * c - loc[:, 1] * s
        p[k:k + per, 1] = box[1] + loc[:, 0] * s + loc[:, 1] * c
        p[k:k + per, 2] = box[2] + loc[:, 2]
        k += per
    p[:, 3] = rng.uniform(0.0, 1.0, n)
    for col in range(4, C - 1):
        p[:, col] = rng.integers(0, 10, n) * 0.25
    return p


def run_reference(case, frames, seed):
    """-> per frame dict(points, gt, ids, draws, visits: ids inside at every get_points_in_box call, flip_x, flip_y)"""
    ref_harness.install()
    from pcdet.datasets.augmentor import augmentor_utils
    from pcdet.datasets.augmentor.data_augmentor import DataAugmentor
    from pcdet.utils import common_utils
    aug = DataAugmentor(None, ref_harness.AttrDict({'DISABLE_AUG_LIST': [], 'AUG_CONFIG_LIST': case['lst']}), ['car'], logger=None)
    draws, visits = [], []
    real_uniform, real_in_box = np.random.uniform, augmentor_utils.get_points_in_box

    def uniform(*a, **k):
        v = real_uniform(*a, **k)
        draws.append(float(v))
        return v

    def in_box(points, box):
        pts, mask = real_in_box(points, box)
        visits.append(points[mask, -1].astype(np.int64))
        return pts, mask

    np.random.uniform, augmentor_utils.get_points_in_box = uniform, in_box
    np.random.seed(seed)
    res = []
    try:
        for f in frames:
            W = f['gt'].shape[1]
            ids = np.arange(f['points'].shape[0], dtype=np.float32)
            pts = f['points'].copy()
            pts[:, -1] = ids
            dd = {'points': pts, 'gt_boxes': f['gt'][:, :W - 1].copy(), 'metadata': {}}
            cls = f['gt'][:, W - 1].copy()
            d0, v0 = len(draws), len(visits)
            for cur, entry in zip(aug.data_augmentor_queue, case['lst']):
                if entry['NAME'] == 'random_world_frustum_dropout' and dd['points'].shape[0] == 0:
                    for _ in entry['DIRECTION']:
                        np.random.uniform(entry['INTENSITY_RANGE'][0], entry['INTENSITY_RANGE'][1])
                    continue
                n_before = dd['gt_boxes'].shape[0]
                if entry['NAME'] == 'random_world_frustum_dropout':                    # follow the class column through the box filter
                    tagged = np.concatenate([dd['gt_boxes'], cls.reshape(-1, 1)], axis=1)
                    dd['gt_boxes'] = tagged
                    dd = cur(data_dict=dd)
                    cls = dd['gt_boxes'][:, -1].copy()
                    dd['gt_boxes'] = dd['gt_boxes'][:, :-1]
                else:
                    dd = cur(data_dict=dd)
                    assert dd['gt_boxes'].shape[0] == n_before
            dd['gt_boxes'][:, 6] = common_utils.limit_period(dd['gt_boxes'][:, 6], offset=0.5, period=2 * np.pi)
            out = np.asarray(dd['points'], dtype=np.float32)
            kept = out[:, -1].astype(np.int64)
            out = out.copy()
            out[:, -1] = f['points'][kept, -1]
            res.append(dict(points=out, ids=kept, gt=np.concatenate([np.asarray(dd['gt_boxes'], np.float32), cls.reshape(-1, 1)], axis=1),
                            draws=np.asarray(draws[d0:], np.float64), visits=visits[v0:], flip_x=bool(dd.get('flip_x', False)),
                            flip_y=bool(dd.get('flip_y', False))))
    finally:
        np.random.uniform, augmentor_utils.get_points_in_box = real_uniform, real_in_box
    return res


def object_input(case, f, r):
    """the frame as it enters the first object entry: the fixture's full list starts with a world rotation, restated here in float32
    through the reference's own rotate_points_along_z"""
    pts, gt = f['points'].copy(), f['gt'].copy()
    if case['lst'][0]['NAME'] == 'random_world_rotation':
        from pcdet.utils import common_utils
        ang = np.array([r['draws'][0]])
        pts[:, :3] = common_utils.rotate_points_along_z(pts[np.newaxis, :, :3], ang)[0]
        gt[:, :3] = common_utils.rotate_points_along_z(gt[np.newaxis, :, :3], ang)[0]
        gt[:, 6] += r['draws'][0]
    return pts, gt


def check_frame(case, f, r, margin):
    """float64 and float32 restatements against the reference -> (bad row ids, measured f32 - f64 difference, smallest distance)"""
    pts, gt = object_input(case, f, r)
    steps, _, _ = oar.steps_of(case['lst'], r['draws'], gt.shape[0])
    log64, log32 = [], []
    _, g64, ids64 = oar.restate_frame(pts, gt, steps, np.float64, log64)
    oar.restate_frame(pts, gt, steps, np.float32, log32)
    bad = np.zeros(pts.shape[0], dtype=bool)
    diff, smallest, same = 0.0, np.inf, True
    local = [v for v in log64 if v['box'] >= 0]
    same &= len(local) == len(r['visits']) and all(np.array_equal(v['inside'], w) for v, w in zip(local, r['visits']))
    same &= np.array_equal(ids64, r['ids']) and g64.shape[0] == r['gt'].shape[0]
    for a, b in zip(log64, log32):
        q = np.abs(a['q'])
        near = np.where(np.isfinite(q), q, np.inf).min(axis=1, initial=np.inf)
        bad[a['ids'][near < margin]] = True
        smallest = min(smallest, float(near.min(initial=np.inf)))
        if 'qb' in a and a['qb'].size:
            smallest = min(smallest, float(np.abs(a['qb']).min()))
            assert np.abs(a['qb']).min() >= margin, 'a box centre within the margin of a world dropout threshold: move the box'
        if a['q'].shape == b['q'].shape and np.array_equal(a['ids'], b['ids']):
            fin = np.isfinite(a['q']) & np.isfinite(b['q'])
            diff = max(diff, float(np.abs(a['q'][fin] - b['q'][fin].astype(np.float64)).max(initial=0.0)))
    return bad, diff, smallest, same, log64


def build_case(case):
    rng = np.random.default_rng(2800 + sum(ord(c) for c in case['name']))
    frames = []
    for n, m in zip(SIZES, N_BOXES):
        gt = make_boxes(rng, m, case['W'])
        frames.append(dict(points=make_rows(rng, n, case['C'], gt), gt=gt))
    margin, measured, redrawn = 1e-4, 0.0, 0
    for _ in range(60):
        res = run_reference(case, frames, case['seed'])
        worst, any_bad, smallest, logs = 0.0, False, np.inf, []
        for f, r in zip(frames, res):
            bad, diff, small, same, log64 = check_frame(case, f, r, margin)
            worst, smallest = max(worst, diff), min(smallest, small)
            logs.append(log64)
            if bad.any():
                any_bad = True
                redrawn += int(bad.sum())
                f['points'][bad] = make_rows(rng, int(bad.sum()), case['C'], f['gt'], only_background=True)
            elif not same:
                raise AssertionError('%s: the float64 restatement and the reference disagree outside the margin' % case['name'])
        measured = max(measured, worst)
        if 10 * measured > margin:
            margin, any_bad = 10 * measured, True
        if not any_bad:
            break
    else:
        raise RuntimeError('conditioning did not converge')
    moved_twice = 0
    if case['name'] in ORDER_DEPENDENT:
        first = [v for v in logs[0] if v['code'] == oar.TRANSLATE_X]
        moved_twice = len(np.intersect1d(first[3]['inside'], first[4]['inside']))
        assert moved_twice > 0, '%s: no row of box 3 lands in box 4' % case['name']
    both = len(np.intersect1d(logs[0][0]['inside'], logs[0][1]['inside'])) if logs[0] and logs[0][0]['box'] == 0 else 0
    return frames, res, dict(margin=margin, measured=measured, smallest=smallest, redrawn=redrawn, moved_twice=moved_twice, in_two_boxes=both)


def collate(case, frames, res):
    def cat(rows):
        return np.concatenate([np.concatenate([np.full((r.shape[0], 1), b, np.float32), r], axis=1) for b, r in enumerate(rows)], axis=0)

    W = case['W']
    out = {'points': cat([f['points'] for f in frames]), 'points_out': cat([r['points'] for r in res])}
    off = np.cumsum([0] + SIZES[:-1])
    out['kept_rows'] = np.concatenate([r['ids'] + o for r, o in zip(res, off)]).astype(np.int64)
    gt, gt_out = np.zeros((len(frames), M_PAD, W), np.float32), np.zeros((len(frames), M_PAD, W), np.float32)
    for b, (f, r) in enumerate(zip(frames, res)):
        gt[b, :f['gt'].shape[0]] = f['gt']
        gt_out[b, :r['gt'].shape[0]] = r['gt']
    out['gt_boxes'], out['gt_boxes_out'] = gt, gt_out
    out['draws'] = np.concatenate([r['draws'] for r in res])
    out['draws_off'] = np.cumsum([0] + [len(r['draws']) for r in res]).astype(np.int64)
    out['flip_x'] = np.asarray([r['flip_x'] for r in res], np.uint8)
    out['flip_y'] = np.asarray([r['flip_y'] for r in res], np.uint8)
    return out


def main():
    arrays, meta = {}, {'pc_range': PC_RANGE, 'sizes': SIZES, 'n_boxes': N_BOXES, 'M': M_PAD, 'cases': {}, 'order_dependent': ORDER_DEPENDENT,
                        'conditioning': {}}
    for case in CASES:
        frames, res, cond = build_case(case)
        for k, v in collate(case, frames, res).items():
            arrays['%s/%s' % (case['name'], k)] = v
        meta['cases'][case['name']] = {'C': case['C'], 'W': case['W'], 'seed': case['seed'], 'cfg': case['lst'],
                                       'kept': [int(r['points'].shape[0]) for r in res], 'boxes_kept': [int(r['gt'].shape[0]) for r in res]}
        meta['conditioning'][case['name']] = cond
        largest = float(np.abs(arrays['%s/points_out' % case['name']][:, 1:4]).max())
        assert largest <= oar.COORD_MAX, largest
        print(case['name'], 'kept', meta['cases'][case['name']]['kept'], 'boxes', meta['cases'][case['name']]['boxes_kept'], cond)
    meta['smallest_margin'] = min(c['margin'] for c in meta['conditioning'].values())
    np.savez_compressed(OUT, meta_json=np.asarray(json.dumps(meta)), **arrays)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
