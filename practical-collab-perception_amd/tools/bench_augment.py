"""Times pcp_world_augment_points (csrc/augment.hip) against the same sequence written in eager torch ops on the GPU.

    python bench_augment.py [--iters 30] [--warmup 5] [--out FILE] [--gt-sampling | --object]

--object times the per-object walk instead (csrc/object_augment.hip through pcp_amd/object_augment.py): 260 000 rows x 1 frame and x 4 frames
of 1 + 5 columns, 40 boxes per frame of (B, 40, 8).  Two lists: moves only (translation x y z, rotation, scaling: 5 sub-stages, one point
launch) and the same plus a local frustum dropout top / left (7 sub-stages, count + place launches and the read of the kept counts).
Timed: pcp_object_augment_points alone on ready box states, local_stages() as a whole (parameter table, box kernel, point kernel), and the
same walk written in torch ops (per frame, sub-stage and box a masked update on the frame's rows; --torch-iters calls, it is slow).

--gt-sampling times the ground-truth database paste instead (csrc/gt_sample.hip through pcp_amd/gt_sampler.py): the nuScenes cloud at
B = 1 and B = 4, the reference's SAMPLE_GROUPS, a synthetic database of 300 objects.  Timed: DeviceGtSampler.apply() with the tile form of
pcp_gt_sample_paste_points (512 output rows staged through LDS), the same with the row-per-thread form (library option gts_paste_form = 1),
the two point-paste launches alone in both forms, the paste followed by the world stages, and the same paste written in torch ops
(torch.cat per frame plus index arithmetic, given the accepted list); all outputs are compared for equality.  GB/s: rows read once plus
rows written once.

Shapes: the nuScenes cloud (260 000 rows and 4 x 260 000 rows of 1 + 12 columns, HD-map layout) and the DiscoNet cloud (4 x 360 000 rows
of 1 + 6 columns).  All stages (flip x, flip y, rotation, scaling, translation) with the range filter on.  CUDA events around every call
after a warm-up, mean over the timed calls; both sides end with the host knowing the kept row count (the kernel path reads 4 B bytes,
the torch path synchronises inside the boolean index).  GB/s counts the useful traffic only: the rows read once plus the kept rows
written once."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from pcp_amd.augment import DeviceWorldAugmentor  # noqa: E402

AUG = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}, {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.7854, 0.7854]},
       {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}, {'NAME': 'random_world_translation', 'NOISE_TRANSLATE_STD': [0.5, 0.5, 0.5]}]
MASK = [{'NAME': 'mask_points_and_boxes_outside_range'}]
SHAPES = [('nuScenes B=1', 1, 260000, 13, True, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]),
          ('nuScenes B=4', 4, 260000, 13, True, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]),
          ('DiscoNet B=4', 4, 360000, 7, False, [-51.2, -51.2, -8.0, 51.2, 51.2, 0.0])]


def make_cloud(B, per_frame, S, hd_map, rng_range, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = B * per_frame
    p = torch.rand(n, S, generator=g)
    p[:, 0] = torch.arange(n) // per_frame
    p[:, 1:3] = (p[:, 1:3] - 0.5) * 2 * 54.0
    p[:, 3] = rng_range[2] - 0.5 + p[:, 3] * (rng_range[5] - rng_range[2] + 1.0)
    if hd_map:
        p[:, 10] = (p[:, 10] - 0.5) * 6.2
    return p.contiguous()


def torch_chain(points, table, B, per_frame, hd_map, rng_range):
    """the reference's per-sample sequence in eager torch ops on the device, frame by frame on row slices, then the range mask"""
    out = points.clone()
    for b in range(B):
        sub = out[b * per_frame:(b + 1) * per_frame]
        fx, fy, c, s, rot, sc = (float(v) for v in table[b, :6])
        t = table[b, 6:9]
        if fx:
            sub[:, 2] *= -1
            if hd_map:
                sub[:, 10] *= -1
        if fy:
            sub[:, 1] *= -1
            if hd_map:
                sub[:, 10] = -(sub[:, 10] + np.pi)
                sub[:, 10] = torch.atan2(torch.sin(sub[:, 10]), torch.cos(sub[:, 10]))
        R = torch.tensor([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]], device=points.device)
        sub[:, 1:4] = torch.matmul(sub[:, 1:4], R)
        if hd_map:
            sub[:, 10] += rot
            sub[:, 10] = torch.atan2(torch.sin(sub[:, 10]), torch.cos(sub[:, 10]))
        sub[:, 1:4] *= sc
        sub[:, 1:4] += t
    r = rng_range
    mask = (out[:, 1] >= r[0]) & (out[:, 1] < r[3]) & (out[:, 2] >= r[1]) & (out[:, 2] < r[4]) & (out[:, 3] >= r[2]) & (out[:, 3] < r[5])
    return out[mask]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return float(ms.mean() * 1e3), float(ms.min() * 1e3)


NUSC_CLASSES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
GT_SAMPLING = {'NAME': 'gt_sampling', 'PREPARE': {'filter_by_min_points': ['%s:5' % c for c in NUSC_CLASSES]},
               'SAMPLE_GROUPS': ['car:2', 'truck:3', 'construction_vehicle:7', 'bus:4', 'trailer:6', 'barrier:2', 'motorcycle:6', 'bicycle:6',
                                 'pedestrian:2', 'traffic_cone:2'],
               'NUM_POINT_FEATURES': 10, 'LIMIT_WHOLE_SCENE': True, 'POINT_FEAT_INDEX_OFFSET_FROM_RAW_FEAT': {'SWEEP_INDEX': 0, 'INSTANCE_INDEX': 1}}
N_SWEEPS = 10


def make_database(n_obj=300, seed=1):
    from pcp_amd.gt_sampler import DeviceGtDatabase
    r = np.random.RandomState(seed)
    cells = r.permutation(21 * 21)[:n_obj]
    boxes = np.zeros((n_obj, 9), np.float32)
    boxes[:, 0], boxes[:, 1] = (cells % 21 - 10) * 4.8 + r.uniform(-0.5, 0.5, n_obj), (cells // 21 - 10) * 4.8 + r.uniform(-0.5, 0.5, n_obj)
    boxes[:, 2] = r.uniform(-2.0, -0.5, n_obj)
    boxes[:, 3:6] = np.stack([r.uniform(0.5, 4.5, n_obj), r.uniform(0.5, 2.2, n_obj), r.uniform(1.0, 2.5, n_obj)], 1)
    boxes[:, 6] = r.uniform(-3.1, 3.1, n_obj)
    boxes[:, 7:9] = r.uniform(-8, 8, (n_obj, 2))
    counts = r.randint(20, 201, n_obj)
    pts = r.uniform(-0.5, 0.5, (int(counts.sum()), 12)).astype(np.float32)
    tf = np.tile(np.eye(4, dtype=np.float32), (n_obj, N_SWEEPS, 1, 1))
    tf[:, :, :3, 3] = r.uniform(-5, 5, (n_obj, N_SWEEPS, 3))
    names = [NUSC_CLASSES[i % 10] for i in range(n_obj)]
    return DeviceGtDatabase(names, boxes, counts, r.uniform(-6, 6, (n_obj, 3)), tf, pts)


def torch_paste(points, per_frame, B, sampler, acc, n_own, cand_box):
    """the same paste in torch ops, given the accepted list acc[b] = (slots, database indices): own rows, then per accepted object its
    stored rows + the box centre with the frame and instance columns set, one torch.cat"""
    db = sampler.db
    parts = []
    for b in range(B):
        parts.append(points[b * per_frame:(b + 1) * per_frame])
        slots, idx = acc[b]
        if idx.numel() == 0:
            continue
        cnt = db.counts_dev[idx].long()
        obj = torch.repeat_interleave(torch.arange(idx.numel(), device=points.device), cnt)
        start = torch.cumsum(cnt, 0) - cnt
        rows = db.offsets_dev[idx].long()[obj] + (torch.arange(obj.numel(), device=points.device) - start[obj])
        new = torch.empty((obj.numel(), points.shape[1]), dtype=torch.float32, device=points.device)
        new[:, 0] = float(b)
        new[:, 1:] = db.points_dev[rows]
        new[:, 1:4] += cand_box[slots][obj, :3]
        new[:, sampler.inst_col] = (n_own[b] + obj).float()
        parts.append(new)
    return torch.cat(parts, 0)


def gt_sampling_bench(args):
    import ctypes
    from pcp_amd import lib
    from pcp_amd.gt_sampler import DeviceGtSampler
    from pcp_amd.ops import _p, _stream
    rr = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    db = make_database()
    lines = ['gt_sampling paste (pcp_gt_sample_select / _paste_points / _paste_boxes), %s, mean (min) of %d calls after %d warm-up calls; database: %d '
             'objects, %d rows of 12 floats' % (torch.cuda.get_device_name(0), args.iters, args.warmup, len(db), int(db.counts.sum()))]
    for B in (1, 4):
        per_frame, S, M = 260000, 13, 30
        sampler = DeviceGtSampler(GT_SAMPLING, NUSC_CLASSES, db)
        aug = DeviceWorldAugmentor([GT_SAMPLING] + AUG, rr, layout='nusc_map', data_processor=MASK, gt_sampler=sampler)
        r = np.random.RandomState(3)
        gt = np.zeros((B, M + 2, 10), np.float32)
        gt[:, :M, 0:2], gt[:, :M, 2] = r.uniform(-50, 50, (B, M, 2)), r.uniform(-2, -0.5, (B, M))
        gt[:, :M, 3:6], gt[:, :M, 6] = r.uniform(0.5, 4.5, (B, M, 3)), r.uniform(-3.1, 3.1, (B, M))
        gt[:, :M, 9] = r.randint(1, 11, (B, M))
        tf = np.tile(np.eye(4, dtype=np.float32)[:3], (B, M + 2, N_SWEEPS, 1, 1))
        glob = np.eye(4)
        glob[:2, :2] = [[np.cos(0.7), -np.sin(0.7)], [np.sin(0.7), np.cos(0.7)]]
        pts = make_cloud(B, per_frame, S, True, rr).cuda()
        batch = {'points': pts, 'gt_boxes': torch.from_numpy(gt).cuda(), 'instances_tf': torch.from_numpy(tf).cuda(), 'batch_size': B,
                 'metadata': [{'tf_target_from_glob': glob} for _ in range(B)]}
        classes = sampler.frame_gt_classes(batch['gt_boxes'])
        params = aug.draw(B, np.random.RandomState(7), classes)
        drawn = params['gt_sampled']
        out = sampler.apply(dict(batch), drawn)
        lib.set_option('gts_paste_form', 1)
        out_rows = sampler.apply(dict(batch), drawn)
        lib.set_option('gts_paste_form', None)
        n_acc = [int(t.numel()) for t in out['gt_sampled_db_index']]
        added = int(out['gt_sampled_rows'].sum())
        ft, cand_db, cand_box, max_added = sampler.candidate_table(drawn, 10, batch['metadata'])
        cand_box_d = torch.from_numpy(cand_box).cuda()
        # the accepted slots for the torch form: database index -> slot inside the frame's candidate range (an index may repeat across frames only)
        acc = []
        for b in range(B):
            idx = out['gt_sampled_db_index'][b].long()
            lo, hi = int(ft[b, 1]), int(ft[b, -1])
            slot_of = {int(d): lo + k for k, d in enumerate(cand_db[lo:hi])}
            acc.append((torch.tensor([slot_of[int(d)] for d in idx.cpu()], dtype=torch.long, device='cuda'), idx))
        n_own = ft[:, 0].tolist()
        want = torch_paste(pts, per_frame, B, sampler, acc, n_own, cand_box_d)
        torch.cuda.synchronize()
        eq_rows, eq_torch = torch.equal(out['points'], out_rows['points']), torch.equal(out['points'], want)
        both = aug.apply(dict(batch), params)
        # the two point-paste launches alone, on the buffers of one prepared call
        G, T = len(sampler.groups), int(cand_db.size)
        dev = pts.device
        ft_d, db_d = torch.from_numpy(ft).to(dev), torch.from_numpy(cand_db).to(dev)
        cap = max(int((ft[:, 1 + G] - ft[:, 1]).max()), 1)
        acc_d = torch.empty((B, cap, lib.GTS_ACC_STRIDE), dtype=torch.int32, device=dev)
        counts = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
        seg = torch.empty(B + 1, dtype=torch.int32, device=dev)
        buf = torch.empty((pts.shape[0] + max_added, S), dtype=torch.float32, device=dev)
        L = lib.load()
        lib.check(L.pcp_gt_sample_select(_p(batch['gt_boxes']), B, M + 2, 10, _p(ft_d), G, _p(db_d), _p(cand_box_d), T, _p(db.counts_dev), len(db), _p(acc_d),
                                         cap, _p(counts), _stream()), 'pcp_gt_sample_select')

        def launches():
            lib.check(L.pcp_gt_sample_paste_points(_p(pts), pts.shape[0], S, B, _p(ft_d), G, _p(acc_d), cap, _p(counts), _p(cand_box_d), _p(db.points_dev),
                                                   _p(db.offsets_dev), sampler.inst_col, max_added, _p(buf), _p(seg), _stream()), 'pcp_gt_sample_paste_points')

        k_us, k_min = timed(launches, args.warmup, args.iters)
        lib.set_option('gts_paste_form', 1)
        r_us, r_min = timed(launches, args.warmup, args.iters)
        a1_us, a1_min = timed(lambda: sampler.apply(dict(batch), drawn), args.warmup, args.iters)
        lib.set_option('gts_paste_form', None)
        a0_us, a0_min = timed(lambda: sampler.apply(dict(batch), drawn), args.warmup, args.iters)
        w_us, w_min = timed(lambda: aug.apply(dict(batch), params), args.warmup, args.iters)
        t_us, t_min = timed(lambda: torch_paste(pts, per_frame, B, sampler, acc, n_own, cand_box_d), args.warmup, args.iters)
        n = B * per_frame
        useful = (n * S + added * 12 + (n + added) * S) * 4
        lines.append('nuScenes B=%d %8d rows x %2d floats, %d candidates, accepted %s, %d rows pasted, outputs equal: tile vs row-per-thread %s, tile vs torch ops %s'
                     % (B, n, S, T, n_acc, added, eq_rows, eq_torch))
        lines.append('  point paste launches alone: LDS tiles %8.1f us (%7.1f) %7.1f GB/s | row per thread %8.1f us (%7.1f) %7.1f GB/s'
                     % (k_us, k_min, useful / k_us / 1e3, r_us, r_min, useful / r_us / 1e3))
        lines.append('  apply() (table, select, paste, one read, boxes): LDS tiles %8.1f us (%7.1f) | row per thread %8.1f us (%7.1f) | torch ops (points only, '
                     'accepted list given) %8.1f us (%7.1f) %6.1f GB/s' % (a0_us, a0_min, a1_us, a1_min, t_us, t_min, useful / t_us / 1e3))
        lines.append('  paste + world stages + range mask: %8.1f us (%7.1f), kept %d of %d rows' % (w_us, w_min, int(both['points'].shape[0]), n + added))
    return lines


def make_boxes(B, M, seed=3):
    """(B, M, 8): M cars on a jittered grid inside +-48 m, any heading"""
    rng = np.random.RandomState(seed)
    g = np.zeros((B, M, 8), dtype=np.float32)
    side = int(np.ceil(np.sqrt(M)))
    for b in range(B):
        for m in range(M):
            g[b, m, 0:2] = (np.array([m % side, m // side]) + 0.5) / side * 96.0 - 48.0 + rng.uniform(-2, 2, 2)
            g[b, m, 2] = rng.uniform(-2.5, -0.5)
            g[b, m, 3:6] = [rng.uniform(3.8, 5.2), rng.uniform(1.7, 2.3), rng.uniform(1.4, 2.0)]
            g[b, m, 6] = rng.uniform(-3.1, 3.1)
            g[b, m, 7] = 1
    return g


def torch_walk(points, gt, stages, values, per_frame):
    """the walk of csrc/object_augment.hip in torch ops on the device: values (B, K, M) float32 CUDA; nothing is read by the host until the
    final boolean index"""
    from pcp_amd import lib as L
    out = points.clone()
    alive = torch.ones(out.shape[0], dtype=torch.bool, device=out.device)
    for b in range(gt.shape[0]):
        sub, al, g = out[b * per_frame:(b + 1) * per_frame], alive[b * per_frame:(b + 1) * per_frame], gt[b].clone()
        for k, st in enumerate(stages):
            for i in range(g.shape[0]):
                box, v = g[i], values[b, k, i]
                sx, sy, sz = sub[:, 1] - box[0], sub[:, 2] - box[1], sub[:, 3] - box[2]
                ca, sa = torch.cos(-box[6]), torch.sin(-box[6])
                lx, ly = sx * ca + sy * (-sa), sx * sa + sy * ca
                m = (sz.abs() <= box[5] / 2) & (lx.abs() <= box[3] / 2 + 0.1) & (ly.abs() <= box[4] / 2 + 0.1) & al
                if st <= L.OBJ_TRANSLATE_Z:
                    sub[:, st] = torch.where(m, sub[:, st] + v, sub[:, st])
                    g[i, st - 1] += v
                elif st == L.OBJ_SCALE:
                    for a, d in ((1, sx), (2, sy), (3, sz)):
                        sub[:, a] = torch.where(m, d * v + box[a - 1], sub[:, a])
                    g[i, 3:6] *= v
                elif st == L.OBJ_ROTATE:
                    c, s_ = torch.cos(v), torch.sin(v)
                    sub[:, 1] = torch.where(m, sx * c - sy * s_ + box[0], sub[:, 1])
                    sub[:, 2] = torch.where(m, sx * s_ + sy * c + box[1], sub[:, 2])
                    g[i, 6] += v
                elif st == L.OBJ_DROP_TOP:
                    al &= ~(m & (sub[:, 3] >= (box[2] + box[5] / 2) - v * box[5]))
                elif st == L.OBJ_DROP_LEFT:
                    al &= ~(m & (sub[:, 2] >= (box[1] + box[4] / 2) - v * box[4]))
    return out[alive]


def object_bench(args):
    import ctypes
    from pcp_amd import lib as L
    from pcp_amd import object_augment as obj
    from pcp_amd.ops import _p, _stream
    moves = [L.OBJ_TRANSLATE_X, L.OBJ_TRANSLATE_Y, L.OBJ_TRANSLATE_Z, L.OBJ_ROTATE, L.OBJ_SCALE]
    lists = [('moves (5 sub-stages)', moves), ('moves + dropout top, left (7 sub-stages)', moves + [L.OBJ_DROP_TOP, L.OBJ_DROP_LEFT])]
    rng_of = {L.OBJ_ROTATE: (-0.3, 0.3), L.OBJ_SCALE: (0.9, 1.1), L.OBJ_DROP_TOP: (0.1, 0.4), L.OBJ_DROP_LEFT: (0.1, 0.4)}
    M, S, per_frame = 40, 6, 260000
    lines = ['pcp_object_augment_points vs the same walk in torch ops, %s, %d boxes per frame, mean (min) of %d calls after %d warm-up calls '
             '(torch ops: %d calls after 1)' % (torch.cuda.get_device_name(0), M, args.iters, args.warmup, args.torch_iters)]
    for B in (1, 4):
        pts = make_cloud(B, per_frame, S, False, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]).cuda()
        gt = torch.from_numpy(make_boxes(B, M)).cuda()
        n = B * per_frame
        for tag, stages in lists:
            rs = np.random.RandomState(5)
            values = [np.stack([rs.uniform(*rng_of.get(st, (-0.5, 0.5)), M) for st in stages]) for _ in range(B)]
            got, g_out, kept = obj.local_stages(pts, gt, stages, values)
            vt = torch.from_numpy(np.stack(values).astype(np.float32)).cuda()
            want = torch_walk(pts, gt, stages, vt, per_frame)
            torch.cuda.synchronize()
            same = got.shape[0] == want.shape[0]
            err = float((got[:, 1:4] - want[:, 1:4]).abs().max()) if same else float('nan')
            # the point kernel alone: box states made once
            a = obj.descriptor(stages, B)
            params = torch.from_numpy(obj.param_table(stages, values, M)).cuda()
            states = torch.empty((B, len(stages), M, L.OBJ_STATE_STRIDE), dtype=torch.float32, device='cuda')
            nb = torch.empty(B, dtype=torch.int32, device='cuda')
            L.check(L.load().pcp_object_augment_boxes(ctypes.byref(a), _p(params), _p(gt.clone()), M, 8, _p(states), _p(nb), _stream()), 'boxes')
            k_us, k_min = timed(lambda: obj._points_call(a, states, nb, M, None, pts), args.warmup, args.iters)
            w_us, w_min = timed(lambda: obj.local_stages(pts, gt, stages, values), args.warmup, args.iters)
            t_us, t_min = timed(lambda: torch_walk(pts, gt, stages, vt, per_frame), 1, args.torch_iters)
            useful = (n + int(got.shape[0])) * S * 4
            lines.append('B=%d %8d rows x %d floats, %s, kept %8d: point kernel %8.1f us (%7.1f) %7.1f GB/s | local_stages() %8.1f us (%7.1f) | '
                         'torch ops %10.1f us (%9.1f) | x%.0f, rows equal %s, max |xyz diff| %.2g'
                         % (B, n, S, tag, got.shape[0], k_us, k_min, useful / k_us / 1e3, w_us, w_min, t_us, t_min, t_us / k_us, same, err))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--gt-sampling', action='store_true', help='time the ground-truth database paste instead of the world stages')
    ap.add_argument('--object', action='store_true', help='time the per-object walk (local moves, local frustum dropouts) instead')
    ap.add_argument('--torch-iters', type=int, default=3, help='--object: timed calls of the torch-ops walk')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_augment.py needs the GPU'
    if args.gt_sampling or args.object:
        text = '\n'.join(object_bench(args) if args.object else gt_sampling_bench(args))
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(text + '\n')
        return
    lines = ['pcp_world_augment_points vs the eager torch-op chain, %s, mean (min) of %d calls after %d warm-up calls'
             % (torch.cuda.get_device_name(0), args.iters, args.warmup)]
    for name, B, per_frame, S, hd_map, rr in SHAPES:
        aug = DeviceWorldAugmentor(AUG, rr, layout='nusc_map' if hd_map else 'disco', data_processor=MASK)
        params = aug.draw(B, np.random.RandomState(7))
        params['flip_x'][:] = True                    # every stage does its work in every frame
        params['flip_y'][:] = True
        table = aug.table(params)
        table_dev = torch.from_numpy(table).cuda()
        table_t = torch.from_numpy(table).cuda()
        pts = make_cloud(B, per_frame, S, hd_map, rr).cuda()
        got, kept = aug.augment_points(pts, table_dev, B)
        want = torch_chain(pts, table_t, B, per_frame, hd_map, rr)
        torch.cuda.synchronize()
        same_rows = got.shape[0] == want.shape[0]
        err = float((got[:, 1:4] - want[:, 1:4]).abs().max()) if same_rows else float('nan')
        k_us, k_min = timed(lambda: aug.augment_points(pts, table_dev, B), args.warmup, args.iters)
        t_us, t_min = timed(lambda: torch_chain(pts, table_t, B, per_frame, hd_map, rr), args.warmup, args.iters)
        n = B * per_frame
        useful = (n + int(got.shape[0])) * S * 4
        lines.append('%-13s %8d rows x %2d floats, kept %8d: kernel %8.1f us (%7.1f) %7.1f GB/s | torch ops %9.1f us (%8.1f) %6.1f GB/s | x%.1f, '
                     'rows equal %s, max |xyz diff| %.2g' % (name, n, S, got.shape[0], k_us, k_min, useful / k_us / 1e3, t_us, t_min, useful / t_us / 1e3,
                                                             t_us / k_us, same_rows, err))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
