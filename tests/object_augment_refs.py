"""numpy restatement of csrc/object_augment.hip (the per-object walk, the frame extent and the world frustum dropout), written from the
behaviour tests/golden/g28_object_augment.npz records.  One frame at a time, sub-stage after sub-stage, box after box; in float32 every
operation is rounded on its own and the rotation's fused multiply-add is the exact float64 product plus the float32 addend rounded once.
With dtype float64 the same walk is the conditioning check of the fixture's generator: `log` then receives, per box visit, the rows
inside and the distance of every row to the nearest face or threshold.  The fixture itself (the reference's own functions) is the first
reference of tests/test_object_augment_cpu.py and tests/test_gpu_object_augment.py; this file is the second."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'g28_object_augment.npz'
F32 = np.float32
TRANSLATE_X, TRANSLATE_Y, TRANSLATE_Z, SCALE, ROTATE = 1, 2, 3, 4, 5           # PCP_OBJ_* of include/pcp_hip_train.h
DROP_TOP, DROP_BOTTOM, DROP_LEFT, DROP_RIGHT = 6, 7, 8, 9
WORLD_DROP_TOP, WORLD_DROP_BOTTOM, WORLD_DROP_LEFT, WORLD_DROP_RIGHT = 10, 11, 12, 13
DIRECTIONS = ('top', 'bottom', 'left', 'right')
OBJECT_NAMES = ('random_local_translation', 'random_local_rotation', 'random_local_scaling', 'random_local_frustum_dropout',
                'random_world_frustum_dropout')
# coordinates: 4 ulp of the largest coordinate magnitude of the fixture (|coords| <= 64), the bound g26 uses; headings 1e-5
COORD_MAX = 64.0
COORD_TOL = 4 * 2.0 ** -23 * COORD_MAX
ANGLE_TOL = 1e-5


def load_fixture():
    z = np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    meta = json.loads(str(d.pop('meta_json')))
    return d, meta


def case_arrays(d, name):
    pre = name + '/'
    return {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}


def sub_stages(cur):
    """[(code, lo, hi)] of one object entry of an AUG_CONFIG_LIST, in the reference's order; [] for a scaling that returns early"""
    name = cur['NAME']
    if name == 'random_local_translation':
        lo, hi = cur['LOCAL_TRANSLATION_RANGE']
        return [({'x': TRANSLATE_X, 'y': TRANSLATE_Y, 'z': TRANSLATE_Z}[a], lo, hi) for a in cur['ALONG_AXIS_LIST']]
    if name == 'random_local_rotation':
        r = cur['LOCAL_ROT_ANGLE']
        lo, hi = r if isinstance(r, (list, tuple)) else (-r, r)
        return [(ROTATE, lo, hi)]
    if name == 'random_local_scaling':
        lo, hi = cur['LOCAL_SCALE_RANGE']
        return [] if hi - lo < 1e-3 else [(SCALE, lo, hi)]
    base = DROP_TOP if name == 'random_local_frustum_dropout' else WORLD_DROP_TOP
    lo, hi = cur['INTENSITY_RANGE']
    return [(base + DIRECTIONS.index(d), lo, hi) for d in cur['DIRECTION']]


def steps_of(aug_list, draws, n_boxes):
    """the object entries of an AUG_CONFIG_LIST with one frame's recorded uniforms (in call order, world rotation / scaling draws
    included) -> ([(code, per-box values | scalar)], uniforms by entry index {qi: array}, the world draws {name: value})"""
    steps, by_entry, world = [], {}, {}
    k = 0
    for qi, cur in enumerate(aug_list):
        name = cur['NAME']
        if name in ('random_world_rotation', 'random_world_scaling'):
            world[name] = float(draws[k])
            k += 1
        if name not in OBJECT_NAMES:
            continue
        vals = []
        for code, _, _ in sub_stages(cur):
            cnt = 1 if code >= WORLD_DROP_TOP else n_boxes
            v = np.asarray(draws[k:k + cnt], dtype=np.float64)
            k += cnt
            steps.append((code, float(v[0]) if code >= WORLD_DROP_TOP else v))
            vals.append(v)
        by_entry[qi] = np.stack(vals) if vals else np.zeros((0, n_boxes))
    return steps, by_entry, world


def cos_sin(angle, dtype):
    if dtype == np.float64:
        return math.cos(angle), math.sin(angle)
    import torch
    a = torch.tensor([angle], dtype=torch.float64).float()         # rotate_points_along_z: the float32 angle through torch.cos / sin
    return F32(torch.cos(a).item()), F32(torch.sin(a).item())


def _fma(a, b, c):
    if a.dtype == np.float64:
        return a * b + c
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)


def in_box(p, box, dtype):
    """get_points_in_box -> (mask, distance of every row to the nearest of the six faces)"""
    sx, sy, sz = p[:, 0] - box[0], p[:, 1] - box[1], p[:, 2] - box[2]
    ca, sa = dtype(math.cos(-float(box[6]))), dtype(math.sin(-float(box[6])))
    lx = sx * ca + sy * (-sa)
    ly = sx * sa + sy * ca
    hx, hy, hz = box[3] / dtype(2.0) + dtype(0.1), box[4] / dtype(2.0) + dtype(0.1), box[5] / dtype(2.0)
    q = np.stack([np.abs(sz) - hz, np.abs(lx) - hx, np.abs(ly) - hy], axis=1)
    return (q <= 0).all(axis=1), q


def restate_frame(points, gt, steps, dtype=F32, log=None):
    """points (n, C) without the frame column, gt (m, W) with the class column, steps from steps_of -> (rows, boxes, ids of the rows kept)"""
    p = points.astype(dtype).copy()
    g = gt.astype(dtype).copy()
    ids = np.arange(p.shape[0])
    for code, vals in steps:
        if code >= WORLD_DROP_TOP:
            if p.shape[0] == 0:                                        # no extent: the frame passes untouched
                continue
            col = 2 if code in (WORLD_DROP_TOP, WORLD_DROP_BOTTOM) else 1
            lo, hi = p[:, col].min(), p[:, col].max()
            upper = code in (WORLD_DROP_TOP, WORLD_DROP_LEFT)
            thr = hi - dtype(vals) * (hi - lo) if upper else lo + dtype(vals) * (hi - lo)
            keep = p[:, col] < thr if upper else p[:, col] > thr
            keep_b = g[:, col] < thr if upper else g[:, col] > thr
            if log is not None:
                log.append(dict(code=code, box=-1, inside=ids[~keep], ids=ids, q=(p[:, col] - thr).reshape(-1, 1), qb=g[:, col] - thr))
            p, ids, g = p[keep], ids[keep], g[keep_b]
            continue
        for i in range(g.shape[0]):
            box = g[i].copy()
            v = dtype(vals[i])
            m, q = in_box(p, box, dtype)
            if log is not None:
                log.append(dict(code=code, box=i, inside=ids[m], ids=ids, q=q))
            if code <= TRANSLATE_Z:
                p[m, code - 1] += v
                g[i, code - 1] += v
            elif code == SCALE:
                for a in range(3):
                    p[m, a] = (p[m, a] - box[a]) * v + box[a]
                g[i, 3:6] *= v
            elif code == ROTATE:
                c, s = cos_sin(float(vals[i]), dtype)
                sx, sy, sz = p[m, 0] - box[0], p[m, 1] - box[1], p[m, 2] - box[2]
                p[m, 0] = _fma(sy, -s, sx * c) + box[0]
                p[m, 1] = _fma(sy, c, sx * s) + box[1]
                p[m, 2] = sz + box[2]
                g[i, 6] += v
            else:
                col, half = (2, box[5]) if code in (DROP_TOP, DROP_BOTTOM) else (1, box[4])
                if code in (DROP_TOP, DROP_LEFT):
                    thr = (box[col] + half / dtype(2)) - v * half
                    dead = m & (p[:, col] >= thr)
                else:
                    thr = (box[col] - half / dtype(2)) + v * half
                    dead = m & (p[:, col] <= thr)
                if log is not None:
                    log[-1]['dead'] = ids[dead]
                    log[-1]['q'] = np.concatenate([q, np.where(m, p[:, col] - thr, np.inf).reshape(-1, 1).astype(q.dtype)], axis=1)
                p, ids = p[~dead], ids[~dead]
    return p, g, ids


def limit_period(h):
    """common_utils.limit_period(h, 0.5, 2 pi) in float32"""
    h = h.astype(F32)
    two_pi = F32(2 * np.pi)
    return (h - np.floor(h / two_pi + F32(0.5)) * two_pi).astype(F32)


def params_of(meta, name, c):
    """the params dict DeviceWorldAugmentor.apply takes, from the recorded draws of a fixture case (queue index = list index: no case has
    a disabled or skipped entry)"""
    cfg = meta['cases'][name]['cfg']
    B = len(meta['sizes'])
    p = {'flip_x': c['flip_x'].astype(bool), 'flip_y': c['flip_y'].astype(bool), 'noise_rot': np.zeros(B), 'noise_scale': np.ones(B),
         'noise_translate': np.zeros((B, 3), F32), 'object': {}}
    for b in range(B):
        _, by_entry, world = steps_of(cfg, c['draws'][c['draws_off'][b]:c['draws_off'][b + 1]], meta['n_boxes'][b])
        p['noise_rot'][b] = world.get('random_world_rotation', 0.0)
        p['noise_scale'][b] = world.get('random_world_scaling', 1.0)
        for qi, v in by_entry.items():
            p['object'].setdefault(qi, [None] * B)[b] = v[:, 0] if cfg[qi]['NAME'] == 'random_world_frustum_dropout' else v
    return p


def flat_draws(cfg, p, b):
    """the uniforms of frame b in call order, from a params dict (the inverse of params_of)"""
    out = []
    for qi, cur in enumerate(cfg):
        if cur['NAME'] == 'random_world_rotation':
            out.append(float(p['noise_rot'][b]))
        elif cur['NAME'] == 'random_world_scaling':
            out.append(float(p['noise_scale'][b]))
        elif cur['NAME'] in OBJECT_NAMES:
            out.extend(np.asarray(p['object'][qi][b], dtype=np.float64).reshape(-1).tolist())
    return np.asarray(out, dtype=np.float64)
