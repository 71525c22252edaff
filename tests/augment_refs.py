"""numpy restatement of the arithmetic of csrc/augment.hip (pcp_world_augment_points / _boxes), written from the behaviour the fixture
tests/golden/g26_augment.npz records: stage after stage in float32, every operation rounded on its own; a fused multiply-add is
restated as the exact float64 product plus the float32 addend, rounded once to float64 and once to float32.  The second reference of
tests/test_augment_cpu.py and tests/test_gpu_augment.py; the first one is the fixture itself (the reference's own functions)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'g26_augment.npz'
FLIP_X, FLIP_Y, ROTATE, SCALE, TRANSLATE = 1, 2, 3, 4, 5           # PCP_AUG_* of include/pcp_hip_train.h
TILE_ROWS = 512                                                   # PCP_AUG_TILE_ROWS: rows one workgroup stages through LDS
F32 = np.float32
PI32 = F32(np.pi)
TWO_PI32 = F32(2 * np.pi)

# bounds of the issue: coordinates, velocities and box sizes 4 ulp of the largest coordinate magnitude of the fixture (|coords| <= 64),
# angles 1e-5, matrices 16 * 2^-24 * max(1, largest |entry|)
COORD_MAX = 64.0
COORD_TOL = 4 * 2.0 ** -23 * COORD_MAX
ANGLE_TOL = 1e-5


def tf_tol(largest):
    return 16 * 2.0 ** -24 * max(1.0, float(largest))


def load_fixture():
    z = np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    meta = json.loads(str(d.pop('meta_json')))
    return d, meta


def case_arrays(d, name):
    pre = name + '/'
    return {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}


def stages_of(aug_list):
    """PCP_AUG_* stage list of an AUG_CONFIG_LIST (world transforms only), in list order"""
    st = []
    for c in aug_list:
        if c['NAME'] == 'random_world_flip':
            st += [FLIP_X if a == 'x' else FLIP_Y for a in c['ALONG_AXIS_LIST']]
        elif c['NAME'] == 'random_world_rotation':
            st.append(ROTATE)
        elif c['NAME'] == 'random_world_scaling':
            st.append(SCALE)
        elif c['NAME'] == 'random_world_translation':
            st.append(TRANSLATE)
    return st


def params_of(c):
    return {'flip_x': c['flip_x'].astype(bool), 'flip_y': c['flip_y'].astype(bool), 'noise_rot': c['noise_rot'], 'noise_scale': c['noise_scale'],
            'noise_translate': c['noise_translate']}


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)


def _rot(x, y, c, s):
    return _fma(y, -F32(s), (x * F32(c)).astype(F32)), _fma(y, F32(c), (x * F32(s)).astype(F32))


def _wrap(v):
    v = v.astype(F32)
    return np.arctan2(np.sin(v), np.cos(v)).astype(F32)


def restate_points(points, table, stages, hd_map, pc_range=None):
    """points (N, 1 + C) float32, table (B, 12) float32 -> (transformed rows, keep mask or None)"""
    out = points.astype(F32).copy()
    S = out.shape[1]
    B = table.shape[0]
    for b in range(B):
        m = out[:, 0] == b
        if not m.any():
            continue
        t = table[b]
        x, y, z = out[m, 1], out[m, 2], out[m, 3]
        lane = out[m, 10] if hd_map else None
        modar = (out[m, S - 3] > 0) if S >= 14 else None
        head = out[m, 9] if S >= 14 else None
        for st in stages:
            if st == FLIP_X and t[0]:
                y = -y
                if hd_map:
                    lane = -lane
                if head is not None:
                    head = np.where(modar, -head, head)
            elif st == FLIP_Y and t[1]:
                x = -x
                if hd_map:
                    lane = _wrap(-(lane + PI32))
                if head is not None:
                    head = np.where(modar, _wrap(-(head + PI32)), head)
            elif st == ROTATE:
                x, y = _rot(x, y, t[2], t[3])
                if hd_map:
                    lane = _wrap(lane + t[4])
                if head is not None:
                    head = np.where(modar, _wrap(head + t[4]), head)
            elif st == SCALE:
                x, y, z = x * t[5], y * t[5], z * t[5]
            elif st == TRANSLATE:
                x, y, z = x + t[6], y + t[7], z + t[8]
        out[m, 1], out[m, 2], out[m, 3] = x, y, z
        if hd_map:
            out[m, 10] = lane
        if head is not None:
            out[m, 9] = head
    if pc_range is None:
        return out, None
    r = np.asarray(pc_range, dtype=F32)
    fb = out[:, 0]
    keep = (fb >= 0) & (fb < B)
    for a in range(3):
        keep &= (out[:, 1 + a] >= r[a]) & (out[:, 1 + a] < r[a + 3])
    return out, keep


def restate_boxes(gt, table, stages):
    """gt (B, M, 8 | 10) float32 -> augmented copy; rows of class 0 untouched"""
    out = gt.astype(F32).copy()
    W = out.shape[2]
    for b in range(out.shape[0]):
        t = table[b]
        real = out[b, :, W - 1] != 0
        g = out[b, real].copy()
        x, y, z, h = g[:, 0], g[:, 1], g[:, 2], g[:, 6]
        dims = g[:, 3:6]
        vx, vy = (g[:, 7], g[:, 8]) if W == 10 else (np.zeros_like(x), np.zeros_like(x))
        for st in stages:
            if st == FLIP_X and t[0]:
                y, h, vy = -y, -h, -vy
            elif st == FLIP_Y and t[1]:
                x, h, vx = -x, -(h + PI32), -vx
            elif st == ROTATE:
                x, y = _rot(x, y, t[2], t[3])
                h = h + t[4]
                vx, vy = _rot(vx, vy, t[2], t[3])
            elif st == SCALE:
                x, y, z, dims, vx, vy = x * t[5], y * t[5], z * t[5], dims * t[5], vx * t[5], vy * t[5]
            elif st == TRANSLATE:
                x, y, z = x + t[6], y + t[7], z + t[8]
        h = (h - np.floor(h / TWO_PI32 + F32(0.5)) * TWO_PI32).astype(F32)
        g[:, 0], g[:, 1], g[:, 2], g[:, 3:6], g[:, 6] = x, y, z, dims, h
        if W == 10:
            g[:, 7], g[:, 8] = vx, vy
        out[b, real] = g
    return out


def restate_tf(tf, gt, table, stages):
    """tf (B, M, S, 3 | 4, 4) float32 -> T A T^-1 per stage as an affine map in float32; matrices of class-0 boxes untouched"""
    out = tf.astype(F32).copy()
    W = gt.shape[2]
    for b in range(out.shape[0]):
        t = table[b]
        real = gt[b, :, W - 1] != 0
        A = out[b, real]
        R, p = A[..., :3, :3].copy(), A[..., :3, 3].copy()
        for st in stages:
            if (st == FLIP_X and t[0]) or (st == FLIP_Y and t[1]):
                ax = 1 if st == FLIP_X else 0
                d = np.ones(3, dtype=F32)
                d[ax] = -1
                R = R * d[:, None] * d[None, :]
                p = p * d
            elif st == ROTATE:
                r0, r1 = _rot(R[..., 0, :], R[..., 1, :], t[2], t[3])
                R = np.stack([r0, r1, R[..., 2, :]], axis=-2)
                c0, c1 = _rot(R[..., :, 0], R[..., :, 1], t[2], t[3])
                R = np.stack([c0, c1, R[..., :, 2]], axis=-1)
                p0, p1 = _rot(p[..., 0], p[..., 1], t[2], t[3])
                p = np.stack([p0, p1, p[..., 2]], axis=-1)
            elif st == SCALE:
                p = (p * t[5]).astype(F32)
            elif st == TRANSLATE:
                d = t[6:9]
                rd = _fma(R[..., 2], d[2], _fma(R[..., 1], d[1], (R[..., 0] * d[0]).astype(F32)))
                p = (p + (d - rd).astype(F32)).astype(F32)
        A[..., :3, :3], A[..., :3, 3] = R, p
        out[b, real] = A
    return out
