"""Generates tests/golden/g27_gt_sampling.npz: the reference's OWN DataBaseSampler (database_sampler.py: __call__,
sample_with_fixed_number, add_sampled_boxes_to_scene) run sample by sample after np.random.seed(s) on a small database this generator
writes to a temporary directory (pickle + .bin files, not committed), with boxes_bev_iou_cpu bound to the reference's iou3d_cpu.cpp
(ref_harness).  Runs only where the reference is mounted; the fixture holds data only: the database arrays, the configs as JSON, the
per-frame inputs and results, and the candidates every sample_with_fixed_number call returned (recorded by wrapping it).

Cases:
  s7    B = 5, rows [x y z i t sweep inst] (NUM_POINT_FEATURES 5), boxes (B, M, 8), instances_tf 4 x 4; 3 classes with 5 / 7 / 3 database
        objects: a short slice at the end of a pass and a second permutation occur; one frame has no boxes, one no points, one is at a
        class's limit
  s12   B = 3, HD-map rows (NUM_POINT_FEATURES 10), boxes (B, M, 10), instances_tf collated to 3 x 4, tf_target_from_glob with a yaw; the
        ten SAMPLE_GROUPS of the reference's nuScenes config; a candidate rejected against an original box, one against a box accepted
        for an earlier class, a mutually rejected pair, at least one accepted per frame.  Second output ('s12/aug_*'): DataAugmentor.forward
        with the gt_sampling entry + flip, rotation, scaling, then mask_points_by_range
  big   B = 2, own rows 511 and 513, more than 1 100 pasted rows per frame, the frame boundary inside a row tile
  prep  B = 2, the database of s7 under PREPARE.filter_by_min_points

Conditioning (checked here, recorded in meta['conditioning']): every candidate x box pair the sampler tests has an overlap area >= 1e-2 m^2
or an axis gap >= 1e-2 m (offending database boxes are redrawn, none is excluded); the rows of the second output keep 1e-4 from the range
bounds (the seed is advanced until they do).  Each listed event is asserted.
"""
import json
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

OUT = os.path.join(HERE, 'g27_gt_sampling.npz')
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
N_SWEEPS = 3
TILE_ROWS = 512
MARGIN = 1e-2
RANGE_MARGIN = 1e-4
CELL = 8.0                     # boxes sit on an 11 x 11 grid of 8 m cells: diagonals stay below 6.5 m, so different cells never touch
NUSC_CLASSES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
NUSC_GROUPS = ['car:2', 'truck:3', 'construction_vehicle:7', 'bus:4', 'trailer:6', 'barrier:2', 'motorcycle:6', 'bicycle:6', 'pedestrian:2',
               'traffic_cone:2']
OFFSETS = {'SWEEP_INDEX': 0, 'INSTANCE_INDEX': 1, 'AUGMENTED_INSTANCE_INDEX': 2, 'CLASS_INDEX': 3}
FLIP = {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}
ROT = {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.3925, 0.3925]}
SCL = {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}

CASES = [
    dict(name='s7', npf=5, W=8, tf_rows=4, classes=['car', 'truck', 'pedestrian'], db_sizes=[5, 7, 3], groups=['car:3', 'truck:2', 'pedestrian:2'],
         frames=[dict(rows=60, gt=['car', 'truck']), dict(rows=45, gt=[]), dict(rows=0, gt=['pedestrian']),
                 dict(rows=70, gt=['car', 'car', 'car', 'truck']), dict(rows=33, gt=['truck'])], prepare={}, seed=3, pts=(5, 40)),
    dict(name='s12', npf=10, W=10, tf_rows=3, classes=NUSC_CLASSES, db_sizes=[3, 4, 8, 4, 7, 3, 6, 7, 2, 3], groups=NUSC_GROUPS,
         frames=[dict(rows=150, gt=['car', 'bus']), dict(rows=90, gt=['truck', 'pedestrian', 'pedestrian']), dict(rows=120, gt=['trailer'])],
         prepare={'filter_by_min_points': ['%s:5' % c for c in NUSC_CLASSES]}, seed=12, pts=(5, 40), aug=True,
         collide=[('orig', 0, 'car', 0), ('db', 'car', 1, 'truck', 0), ('db', 'construction_vehicle', 0, 'construction_vehicle', 1)]),
    dict(name='big', npf=5, W=8, tf_rows=4, classes=['car', 'truck', 'pedestrian'], db_sizes=[25, 25, 25],
         groups=['car:25', 'truck:25', 'pedestrian:25'], frames=[dict(rows=511, gt=['car']), dict(rows=513, gt=['truck', 'car'])], prepare={}, seed=5,
         pts=(24, 40)),
    dict(name='prep', npf=5, W=8, tf_rows=4, classes=['car', 'truck', 'pedestrian'], db_sizes=[5, 7, 3], groups=['car:3', 'truck:2', 'pedestrian:2'],
         frames=[dict(rows=20, gt=['car']), dict(rows=25, gt=[])], prepare={'filter_by_min_points': ['car:20', 'truck:12', 'pedestrian:0']}, seed=9,
         pts=(5, 40), db_of='s7'),
]


def yaw_tf(yaw, t):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = t
    return T


class Cells:
    """hands out grid cells, each once"""

    def __init__(self, rng):
        self.free = [(i, j) for i in range(-5, 6) for j in range(-5, 6)]
        rng.shuffle(self.free)

    def centre(self, rng):
        i, j = self.free.pop()
        return np.array([i * CELL + rng.uniform(-0.5, 0.5), j * CELL + rng.uniform(-0.5, 0.5)])


def make_box(rng, xy, width):
    b = np.zeros(width, dtype=np.float32)
    b[0:2] = xy
    b[2] = rng.uniform(-2.0, -0.5)
    b[3:6] = [rng.uniform(1.5, 4.5), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.5)]
    b[6] = rng.uniform(-3.1, 3.1)
    if width == 9:
        b[7:9] = rng.uniform(-8, 8, 2)
    return b


def make_rows(rng, n, npf, spread):
    """n rows of npf + 2 columns; spread: None = scene rows over the range and beyond, else a box's (dx, dy, dz) for centred object rows"""
    p = np.zeros((n, npf + 2), dtype=np.float32)
    if spread is None:
        p[:, 0:2] = rng.uniform(-56.0, 56.0, (n, 2))
        p[:, 2] = rng.uniform(-6.0, 4.0, n)
    else:
        p[:, 0:3] = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(spread, dtype=np.float64)
    p[:, 3] = rng.uniform(0.0, 1.0, n)
    p[:, 4] = rng.integers(0, 10, n) * 0.05
    if npf == 10:
        p[:, 5:9] = rng.uniform(0, 1, (n, 4)) < 0.3
        p[:, 9] = rng.uniform(-3.0, 3.0, n)
    p[:, npf] = rng.integers(0, N_SWEEPS, n)
    p[:, npf + 1] = rng.integers(-1, 9, n)
    return p


def make_tfs(rng, m):
    tf = np.zeros((m, N_SWEEPS, 4, 4), dtype=np.float32)
    for i in range(m):
        for s in range(N_SWEEPS):
            tf[i, s] = yaw_tf(rng.uniform(-0.4, 0.4), rng.uniform(-8, 8, 3))
    return tf


def make_database(case, rng, cells):
    """-> list of records in uid order (classes in order, objects in order) and the per-object rows"""
    recs, rows = [], []
    for cname, size in zip(case['classes'], case['db_sizes']):
        for k in range(size):
            box = make_box(rng, cells.centre(rng), case['W'] - 1)
            n = int(rng.integers(case['pts'][0], case['pts'][1] + 1))
            recs.append({'name': cname, 'box3d_lidar': box, 'num_points_in_gt': n, 'instance_tf': make_tfs(rng, 1)[0],
                         'velo': rng.uniform(-6, 6, 3), 'uid': len(recs), 'path': 'gt_database/%d.bin' % len(recs), 'difficulty': 0, 'k': k})
            rows.append(make_rows(rng, n, case['npf'], box[3:6]))
    return recs, rows


def make_frames(case, rng, cells):
    frames = []
    for b, f in enumerate(case['frames']):
        m = len(f['gt'])
        gt = np.stack([make_box(rng, cells.centre(rng), case['W'] - 1) for _ in range(m)]) if m else np.zeros((0, case['W'] - 1), np.float32)
        frames.append(dict(points=make_rows(rng, f['rows'], case['npf'], None), gt=gt, names=np.array(f['gt'], dtype='<U32'), tf=make_tfs(rng, m),
                           glob=yaw_tf(0.6 + 0.35 * b, [12.0 * b, -30.0 + b, 0.4])))
    return frames


def apply_collisions(case, recs, frames):
    """moves database boxes so that the listed events occur: ('orig', frame, class, k): object k of the class overlaps the frame's first box;
    ('db', class a, ka, class b, kb): object kb of b overlaps object ka of a"""
    def rec(cname, k):
        return next(r for r in recs if r['name'] == cname and r['k'] == k)
    for ev in case.get('collide', []):
        if ev[0] == 'orig':
            rec(ev[2], ev[3])['box3d_lidar'][0:2] = frames[ev[1]]['gt'][0, 0:2] + np.float32([0.8, 0.4])
        else:
            rec(ev[3], ev[4])['box3d_lidar'][0:2] = rec(ev[1], ev[2])['box3d_lidar'][0:2] + np.float32([0.7, -0.3])


def write_database(root, recs, rows):
    os.makedirs(os.path.join(root, 'gt_database'), exist_ok=True)
    infos = {}
    for r, p in zip(recs, rows):
        p.astype(np.float32).tofile(os.path.join(root, r['path']))
        infos.setdefault(r['name'], []).append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()})
    with open(os.path.join(root, 'dbinfos.pkl'), 'wb') as f:
        pickle.dump(infos, f)


def sampler_cfg(case):
    return {'NAME': 'gt_sampling', 'DB_INFO_PATH': ['dbinfos.pkl'], 'PREPARE': case['prepare'], 'SAMPLE_GROUPS': case['groups'],
            'NUM_POINT_FEATURES': case['npf'], 'DATABASE_WITH_FAKELIDAR': False, 'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True,
            'POINT_FEAT_INDEX_OFFSET_FROM_RAW_FEAT': OFFSETS}


def gap_of(a, b):
    """largest separation of two BEV rectangles over their four face normals (float64); < 0: they overlap"""
    def corners(q):
        c, s = np.cos(q[6]), np.sin(q[6])
        d = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]]) * np.array([q[3], q[4]]) / 2.0
        return d @ np.array([[c, s], [-s, c]]) + q[0:2]
    ca, cb = corners(np.asarray(a, np.float64)), corners(np.asarray(b, np.float64))
    best = -np.inf
    for q in (a, b):
        for ang in (q[6], q[6] + np.pi / 2):
            ax = np.array([np.cos(ang), np.sin(ang)])
            pa, pb = ca @ ax, cb @ ax
            best = max(best, pa.min() - pb.max(), pb.min() - pa.max())
    return best


def run_reference(case, recs, rows, frames, seed, with_aug=False):
    """-> per frame results; events; uids of the database boxes that miss the conditioning"""
    ref_harness.install()
    import torch
    from pcdet.datasets.augmentor.data_augmentor import DataAugmentor
    from pcdet.datasets.augmentor.database_sampler import DataBaseSampler
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    from pcdet.utils import common_utils
    with tempfile.TemporaryDirectory() as root:
        write_database(root, recs, rows)
        cfg = ref_harness.AttrDict(sampler_cfg(case))
        if with_aug:
            aug = DataAugmentor(Path(root), ref_harness.AttrDict({'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': [sampler_cfg(case), FLIP, ROT, SCL]}),
                                case['classes'], logger=None)
            sampler = aug.data_augmentor_queue[0]
        else:
            sampler = DataBaseSampler(Path(root), cfg, case['classes'], logger=None)
        log = {'cands': [], 'accepted': [], 'short': 0, 'permutations': {}}
        real_fixed, real_add, real_perm = sampler.sample_with_fixed_number, sampler.add_sampled_boxes_to_scene, np.random.permutation
        cur = {}

        def fixed(class_name, sample_group):
            cur['class'] = class_name
            got = real_fixed(class_name, sample_group)
            log['cands'][-1][class_name] = [int(x['uid']) for x in got]
            log['short'] += len(got) < int(sample_group['sample_num'])
            return got

        def add(data_dict, boxes, total, *a, **k):
            log['accepted'][-1] = [int(x['uid']) for x in total]
            return real_add(data_dict, boxes, total, *a, **k)

        def perm(n):
            log['permutations'][cur['class']] = log['permutations'].get(cur['class'], 0) + 1
            return real_perm(n)

        sampler.sample_with_fixed_number, sampler.add_sampled_boxes_to_scene, np.random.permutation = fixed, add, perm
        np.random.seed(seed)
        res = []
        try:
            for f in frames:
                log['cands'].append({})
                log['accepted'].append([])
                dd = {'points': f['points'].copy(), 'gt_boxes': f['gt'].copy(), 'gt_names': f['names'].copy(), 'instances_tf': f['tf'].copy(),
                      'gt_boxes_mask': np.ones(len(f['names']), dtype=bool), 'metadata': {'tf_target_from_glob': f['glob'].copy(), 'use_hd_map': case['npf'] == 10}}
                dd = aug.forward(dd) if with_aug else sampler(dd)
                cls = np.array([case['classes'].index(n) + 1 for n in dd['gt_names']], dtype=np.float32).reshape(-1, 1)
                r = dict(points=np.asarray(dd['points'], dtype=np.float32), gt=np.concatenate([np.asarray(dd['gt_boxes'], dtype=np.float32), cls], axis=1),
                         tf=np.asarray(dd['instances_tf']), added=int(dd['metadata'].get('num_added_instances', 0)))
                assert dd['points'].dtype == np.float32 and r['added'] == len(log['accepted'][-1])
                if with_aug:
                    r.update(mask=np.asarray(common_utils.mask_points_by_range(dd['points'], PC_RANGE), dtype=bool), flip_x=bool(dd['flip_x']),
                             flip_y=bool(dd['flip_y']), noise_rot=float(dd['noise_rot']), noise_scale=float(dd['noise_scale']))
                res.append(r)
        finally:
            np.random.permutation = real_perm
    # replay the decisions with the reference's IoU: which events occurred, which pairs are badly conditioned
    by_uid = {r['uid']: r for r in recs}
    events = {'vs_original': 0, 'vs_earlier_class': 0, 'mutual': 0, 'accepted_per_frame': [len(a) for a in log['accepted']],
              'short': int(log['short']), 'permutations': log['permutations'], 'limit_skips': 0}
    bad = set()
    if not with_aug:
        for f, cands, acc in zip(frames, log['cands'], log['accepted']):
            existed = [np.asarray(g[:7], np.float32) for g in f['gt']]
            n_orig = len(existed)
            for g in case['groups']:
                cname = g.split(':')[0]
                if cname not in cands:
                    events['limit_skips'] += 1
                    continue
                cb = [by_uid[u]['box3d_lidar'][:7].astype(np.float32) for u in cands[cname]]
                others = existed + cb
                iou = iou3d_nms_utils.boxes_bev_iou_cpu(np.stack(cb), np.stack(others))
                for i, u in enumerate(cands[cname]):
                    hit_o = hit_e = hit_m = False
                    for j, o in enumerate(others):
                        if j == len(existed) + i:
                            continue
                        sa, sb = float(cb[i][3] * cb[i][4]), float(o[3] * o[4])
                        area = iou[i, j] * (sa + sb) / (1.0 + iou[i, j])
                        gap = gap_of(cb[i], o)
                        if not (area >= MARGIN or (iou[i, j] == 0 and gap >= MARGIN)):
                            bad.add(u)
                        if iou[i, j] > 0:
                            hit_o |= j < n_orig
                            hit_e |= n_orig <= j < len(existed)
                            hit_m |= j >= len(existed)
                    assert (u in acc) == (not (hit_o or hit_e or hit_m)), (u, hit_o, hit_e, hit_m)
                    events['vs_original'] += hit_o
                    events['vs_earlier_class'] += hit_e and not hit_o
                    events['mutual'] += hit_m
                existed = existed + [by_uid[u]['box3d_lidar'][:7].astype(np.float32) for u in cands[cname] if u in acc]
    return res, log, events, bad


def collate(case, frames, res, key_prefix=''):
    B, S, W, R = len(frames), case['npf'] + 3, case['W'], case['tf_rows']

    def cat(rows):
        return np.concatenate([np.concatenate([np.full((r.shape[0], 1), b, np.float32), r], axis=1) for b, r in enumerate(rows)], axis=0).reshape(-1, S)

    def boxes(gts, m):
        out = np.zeros((B, m, W), np.float32)
        for b, g in enumerate(gts):
            out[b, :g.shape[0]] = g
        return out

    def tfs(ts, m, dtype):
        out = np.zeros((B, m, N_SWEEPS, R, 4), dtype)
        out[..., :3, :3] = np.eye(3)
        for b, t in enumerate(ts):
            out[b, :t.shape[0]] = t[..., :R, :]
        return out

    out = {}
    if not key_prefix:
        M = max(f['gt'].shape[0] for f in frames) + 2            # two padding rows even behind the longest frame
        cls = [np.array([case['classes'].index(n) + 1 for n in f['names']], np.float32).reshape(-1, 1) for f in frames]
        out.update(points=cat([f['points'] for f in frames]), gt_boxes=boxes([np.concatenate([f['gt'], c], axis=1) for f, c in zip(frames, cls)], M),
                   instances_tf=tfs([f['tf'] for f in frames], M, np.float32), tf_target_from_glob=np.stack([f['glob'] for f in frames]))
    m_out = max(r['gt'].shape[0] for r in res)
    out[key_prefix + 'points_out'] = cat([r['points'] for r in res])
    out[key_prefix + 'gt_boxes_out'] = boxes([r['gt'] for r in res], m_out)
    out[key_prefix + 'instances_tf_out'] = tfs([r['tf'] for r in res], m_out, np.float64 if key_prefix else np.float32)
    out[key_prefix + 'added'] = np.asarray([r['added'] for r in res], dtype=np.int64)
    if key_prefix:
        out[key_prefix + 'mask'] = np.concatenate([r['mask'] for r in res])
        for key, dt in (('flip_x', np.uint8), ('flip_y', np.uint8), ('noise_rot', np.float64), ('noise_scale', np.float64)):
            out[key_prefix + key] = np.asarray([r[key] for r in res], dtype=dt)
    return out


def build_case(case, databases):
    rng = np.random.default_rng(2700 + 31 * len(case['name']) + case['npf'])
    cells = Cells(rng)
    if 'db_of' in case:
        recs, rows = databases[case['db_of']]
        recs = [dict(r, box3d_lidar=r['box3d_lidar'].copy()) for r in recs]
        for _ in recs:
            cells.free.pop()
    else:
        recs, rows = make_database(case, rng, cells)
    frames = make_frames(case, rng, cells)
    apply_collisions(case, recs, frames)
    redrawn = 0
    for _ in range(20):
        res, log, events, bad = run_reference(case, recs, rows, frames, case['seed'])
        if not bad:
            break
        for u in bad:                                          # redraw the box's place, keep the object
            recs[u]['box3d_lidar'][0:2] = Cells.centre(cells, rng)
            redrawn += 1
    else:
        raise RuntimeError('conditioning did not converge')
    return recs, rows, frames, res, log, events, redrawn


def main():
    arrays, meta = {}, {'pc_range': PC_RANGE, 'n_sweeps': N_SWEEPS, 'tile_rows': TILE_ROWS, 'cases': {},
                        'conditioning': {'margin': MARGIN, 'range_margin': RANGE_MARGIN, 'redrawn': {}}}
    databases = {}
    for case in CASES:
        name = case['name']
        recs, rows, frames, res, log, events, redrawn = build_case(case, databases)
        databases[name] = (recs, rows)
        c = collate(case, frames, res)
        c.update(db_boxes=np.stack([r['box3d_lidar'] for r in recs]).astype(np.float32), db_counts=np.asarray([r['num_points_in_gt'] for r in recs], np.int64),
                 db_velo=np.stack([r['velo'] for r in recs]).astype(np.float64), db_instance_tf=np.stack([r['instance_tf'] for r in recs]).astype(np.float32),
                 db_points=np.concatenate(rows, axis=0).astype(np.float32))
        info = {'npf': case['npf'], 'W': case['W'], 'tf_rows': case['tf_rows'], 'classes': case['classes'], 'seed': case['seed'], 'sampler_cfg': sampler_cfg(case),
                'db_names': [r['name'] for r in recs], 'own_rows': [int(f['points'].shape[0]) for f in frames], 'n_own': [int(f['gt'].shape[0]) for f in frames],
                'candidates': log['cands'], 'accepted': log['accepted'], 'events': ref_harness.to_plain(events),
                'added_rows': [int(r['points'].shape[0] - f['points'].shape[0]) for r, f in zip(res, frames)]}
        # the listed events, asserted so that a reseed cannot silently lose one
        if name == 's7':
            assert events['short'] >= 1 and max(events['permutations'].values()) >= 2 and events['limit_skips'] >= 1, events
            assert 0 in info['n_own'] and 0 in info['own_rows']
            assert any(len(v) < int(g.split(':')[1]) for cands in log['cands'] for g in case['groups'] for k, v in cands.items() if k == g.split(':')[0])
        if name == 's12':
            assert events['vs_original'] >= 1 and events['vs_earlier_class'] >= 1 and events['mutual'] >= 2 and min(events['accepted_per_frame']) >= 1, events
            assert float(np.abs(frames[0]['glob'][:2, :2] - np.eye(2)).max()) > 0.3
            for seed in range(case['seed'], case['seed'] + 50):
                ares, alog, _, _ = run_reference(case, recs, rows, frames, seed, with_aug=True)
                lim = np.asarray(PC_RANGE)
                ok = True
                for r in ares:
                    p = r['points'][:, :3].astype(np.float64)
                    ok &= all((np.abs(p[:, a] - lim[a]) >= RANGE_MARGIN).all() and (np.abs(p[:, a] - lim[a + 3]) >= RANGE_MARGIN).all() for a in range(3))
                    ok &= bool((np.abs(np.abs(r['gt'][:, 6].astype(np.float64)) - np.pi) >= RANGE_MARGIN).all())
                    ok &= bool((np.abs(np.abs(r['points'][:, 9].astype(np.float64)) - np.pi) >= RANGE_MARGIN).all())
                    ok &= float(np.abs(p).max(initial=0.0)) <= 64.0
                if ok and min(len(a) for a in alog['accepted']) >= 1:
                    break
            else:
                raise RuntimeError('no seed conditions the augmented rows')
            c.update(collate(case, frames, ares, key_prefix='aug_'))
            info.update(aug_seed=seed, aug_cfg={'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': [sampler_cfg(case), FLIP, ROT, SCL]},
                        aug_candidates=alog['cands'], aug_accepted=alog['accepted'], aug_kept=[int(r['mask'].sum()) for r in ares],
                        largest_tf=float(max(np.abs(r['tf']).max() for r in ares)))
        if name == 'big':
            first = info['own_rows'][0] + info['added_rows'][0]
            assert info['own_rows'] == [511, 513] and max(info['added_rows']) > 1100 and first % TILE_ROWS not in (0, 1, TILE_ROWS - 1), info['added_rows']
            assert (first + info['own_rows'][1] + info['added_rows'][1]) // TILE_ROWS >= 4
        if name == 'prep':
            kept = {cn: [r['uid'] for r in recs if r['name'] == cn and r['num_points_in_gt'] >= int(n)] for cn, n in
                    (x.split(':') for x in case['prepare']['filter_by_min_points'])}
            assert any(0 < len(v) < sum(r['name'] == cn for r in recs) for cn, v in kept.items()), kept
            assert all(u in kept[cn] for cands in log['cands'] for cn, us in cands.items() for u in us)
        meta['cases'][name] = info
        meta['conditioning']['redrawn'][name] = redrawn
        for k, v in c.items():
            arrays['%s/%s' % (name, k)] = v
        print(name, 'rows', c['points'].shape, '->', c['points_out'].shape, 'added', info['added_rows'], 'accepted', events['accepted_per_frame'],
              'events', {k: v for k, v in events.items() if k != 'accepted_per_frame'}, 'redrawn', redrawn)
    np.savez_compressed(OUT, meta_json=np.asarray(json.dumps(meta)), **arrays)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
