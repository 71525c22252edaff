"""Restatements the hard-voxelisation and PillarVFE tests compare against (no test in this file).

hard_voxelize_ref: spconv's CPU point-to-voxel generator (C++ 1.2 and 2.x; spconv itself is not installable offline), the loop the
reference's transform_points_to_voxels runs per frame (pcdet/datasets/processor/data_processor.py:116-144), in numpy with float32
operations, applied frame by frame to collated rows and concatenated the way collate_batch leaves the three tensors.

pillar_vfe_ref: pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-123 with one PFN layer, in float64.
"""
import numpy as np


def grid_of(pc_range, voxel_size):
    r = np.asarray(pc_range, dtype=np.float32)
    return np.round((r[3:6] - r[0:3]) / np.asarray(voxel_size, dtype=np.float32)).astype(np.int64)


def hard_voxelize_frame(pts, pc_range, voxel_size, max_points, max_voxels):
    """pts (n, C) float32 [x, y, z, f...] of ONE frame -> voxels (M, T, C) float32, coords (M, 3) int32 [z, y, x], num (M,) int32"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    rmin = np.asarray(pc_range, dtype=np.float32)[:3]
    vs = np.asarray(voxel_size, dtype=np.float32)
    grid = grid_of(pc_range, voxel_size)
    c = np.floor((pts[:, :3] - rmin[None, :]) / vs[None, :])                    # float32 subtract, float32 IEEE divide, floor
    assert c.dtype == np.float32
    table = {}
    voxels = np.zeros((max_voxels if max_voxels < pts.shape[0] else max(pts.shape[0], 1), max_points, pts.shape[1]), dtype=np.float32)
    coords, num = [], []
    for i in range(pts.shape[0]):
        ci = c[i]
        if (ci[0] < 0 or ci[0] >= grid[0] or ci[1] < 0 or ci[1] >= grid[1] or ci[2] < 0 or ci[2] >= grid[2]):
            continue
        key = (int(ci[2]), int(ci[1]), int(ci[0]))
        v = table.get(key, -1)
        if v == -1:
            if len(coords) >= max_voxels:
                continue
            v = len(coords)
            table[key] = v
            coords.append(key)
            num.append(0)
        if num[v] < max_points:
            voxels[v, num[v]] = pts[i]
            num[v] += 1
    M = len(coords)
    return voxels[:M].copy(), np.asarray(coords, dtype=np.int32).reshape(M, 3), np.asarray(num, dtype=np.int32)


def hard_voxelize_ref(points, pc_range, voxel_size, max_points, max_voxels, batch_size):
    """points (N, 1 + C) collated rows -> voxels (M, T, C), voxel_coords (M, 4) int32 [b, z, y, x], voxel_num_points (M,) int32,
    voxels per frame (list of batch_size ints); frames concatenated in frame order"""
    points = np.asarray(points, dtype=np.float32)
    vox, crd, num, per = [], [], [], []
    for b in range(batch_size):
        v, c, k = hard_voxelize_frame(points[points[:, 0] == b][:, 1:], pc_range, voxel_size, max_points, max_voxels)
        vox.append(v)
        crd.append(np.concatenate([np.full((c.shape[0], 1), b, dtype=np.int32), c], 1))
        num.append(k)
        per.append(int(k.shape[0]))
    return (np.concatenate(vox, 0).reshape(-1, max_points, points.shape[1] - 1), np.concatenate(crd, 0).astype(np.int32).reshape(-1, 4),
            np.concatenate(num, 0).astype(np.int32), per)


def pillar_vfe_ref(voxels, num, coords, voxel_size, offset, w, b, use_absolute_xyz=True, with_distance=False):
    """float64 PillarVFE with one PFN layer; w (out, K), b (out,): Linear with the BatchNorm folded.  Returns (M, out) float64."""
    v = np.asarray(voxels, dtype=np.float64)
    n = np.asarray(num, dtype=np.float64)
    M, T, _C = v.shape
    mean = v[:, :, :3].sum(1, keepdims=True) / n.reshape(-1, 1, 1)
    f_cluster = v[:, :, :3] - mean
    f_center = np.zeros_like(v[:, :, :3])
    for j, col in enumerate((3, 2, 1)):                                           # x <- coords[:, 3], y <- coords[:, 2], z <- coords[:, 1]
        f_center[:, :, j] = v[:, :, j] - (coords[:, col].astype(np.float64)[:, None] * float(np.float32(voxel_size[j])) + float(np.float32(offset[j])))
    feats = [v if use_absolute_xyz else v[:, :, 3:], f_cluster, f_center]
    if with_distance:
        feats.append(np.sqrt((v[:, :, :3] ** 2).sum(2, keepdims=True)))
    f = np.concatenate(feats, -1)
    f = f * (np.arange(T)[None, :] < np.asarray(num)[:, None]).astype(np.float64)[:, :, None]
    y = f @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    return np.maximum(y, 0.0).max(1)


def fold_bn(w, gamma, beta, mean, var, eps=1e-3):
    """float64 fold of BatchNorm1d(eval) into the Linear in front of it"""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return np.asarray(w, np.float64) * s[:, None], np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * s
