"""Times the classic PointPillar front end on the device: hard_voxelize, pcp_pillar_vfe, and the two together beside a restatement in torch
ops on the same device.  HIP events around each call, 5 warm-up calls, mean and minimum of 30.

    python tools/bench_hard_voxel.py [--out ../../profiles/hard_voxel_bench.txt]

Clouds: the synthetic car cloud of bench.py (7 point features, +-52 m), frames of 60 000 and 260 000 rows, B = 1 and 4, uniform and ring.
Voxeliser: the settings of v2x_pointpillar_anchor_hardvoxel.yaml (0.2 m pillars on 512 x 512, T = 32, at most 40 000 voxels per frame).
The torch-ops restatement (stable sort by cell, first index per cell, rank by first index; then the reference's dense PillarVFE arithmetic on
the padded (M, T, C) tensor) is checked against the kernels before it is timed.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))

from pcp_amd import ops, synth  # noqa: E402

PC_RANGE = [-51.2, -51.2, -8.0, 51.2, 51.2, 0.0]
VOXEL = [0.2, 0.2, 8.0]
GRID = [512, 512, 1]
T, MAX_VOXELS, OUT = 32, 40000, 64
WARMUP, RUNS = 5, 30


def make_cloud(rows, batch, dist):
    frames = []
    for f in range(batch):
        parts, a = [], 0
        while sum(p.shape[0] for p in parts) < rows:
            parts.append(synth.agent_cloud(agent=10 * f + a, n_points=60000, layout='car', dist=dist))
            a += 1
        frames.append(np.concatenate(parts, 0)[:rows])
    return torch.from_numpy(synth.collate(frames)).cuda()


def torch_hard_voxelize(points, batch):
    """hard voxelisation in torch ops: the same voxel numbers and slots as the generator's loop"""
    dev = points.device
    rmin = torch.tensor(PC_RANGE[:3], dtype=torch.float32, device=dev)
    vs = torch.tensor(VOXEL, dtype=torch.float32, device=dev)
    c = torch.floor((points[:, 1:4] - rmin) / vs)
    g = torch.tensor(GRID, dtype=torch.float32, device=dev)
    ok = ((c >= 0) & (c < g)).all(1)
    rows = torch.nonzero(ok)[:, 0]
    b = points[rows, 0].long()
    ci = c[rows].long()
    cell = (b * GRID[1] + ci[:, 1]) * GRID[0] + ci[:, 0]
    order = torch.argsort(cell, stable=True)                       # rows of a cell together, in input order
    cs = cell[order]
    uniq, counts = torch.unique_consecutive(cs, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    first_row = rows[order][start]                                 # smallest input index of every cell
    by_first = torch.argsort(first_row)                            # first appearance (frames are grouped, so frame-major)
    fb = uniq[by_first] // (GRID[0] * GRID[1])
    per_frame = torch.bincount(fb, minlength=batch)
    frame_start = torch.cumsum(per_frame, 0) - per_frame
    rank_in_frame = torch.arange(by_first.numel(), device=dev) - frame_start[fb]
    kept = by_first[rank_in_frame < MAX_VOXELS]
    M = int(kept.numel())                                          # the one host read
    vox_of_cell = torch.full((uniq.numel(),), -1, dtype=torch.long, device=dev)
    vox_of_cell[kept] = torch.arange(M, device=dev)
    seg = torch.repeat_interleave(torch.arange(uniq.numel(), device=dev), counts)
    slot = torch.arange(cs.numel(), device=dev) - start[seg]
    v = vox_of_cell[seg]
    take = (v >= 0) & (slot < T)
    voxels = torch.zeros((M, T, points.shape[1] - 1), dtype=torch.float32, device=dev)
    voxels[v[take], slot[take]] = points[rows[order][take], 1:]
    ku = uniq[kept]
    rem = ku % (GRID[0] * GRID[1])
    coords = torch.stack([ku // (GRID[0] * GRID[1]), torch.zeros_like(ku), rem // GRID[0], rem % GRID[0]], 1).int()
    num = torch.clamp(counts[kept], max=T).int()
    return voxels, coords, num


def torch_pillar_vfe(voxels, num, coords, w, b, offset):
    mean = voxels[:, :, :3].sum(1, keepdim=True) / num.type_as(voxels).view(-1, 1, 1)
    f_cluster = voxels[:, :, :3] - mean
    f_center = torch.zeros_like(voxels[:, :, :3])
    for j, col in enumerate((3, 2, 1)):
        f_center[:, :, j] = voxels[:, :, j] - (coords[:, col].to(voxels.dtype).unsqueeze(1) * VOXEL[j] + offset[j])
    f = torch.cat([voxels, f_cluster, f_center], -1)
    mask = (num.view(-1, 1) > torch.arange(voxels.shape[1], device=voxels.device).view(1, -1)).unsqueeze(-1).type_as(voxels)
    f = f * mask
    return torch.relu(f @ w.t() + b).max(1)[0]


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = ['hard voxelisation + PillarVFE (T = %d, at most %d voxels per frame, %d channels), milliseconds: mean (min) of %d after %d warm-up calls'
             % (T, MAX_VOXELS, OUT, RUNS, WARMUP),
             '%-8s %2s %8s %8s | %16s %16s %16s %18s' % ('cloud', 'B', 'rows', 'voxels', 'hard_voxelize', 'pcp_pillar_vfe', 'both', 'both, torch ops')]
    rs = np.random.RandomState(0)
    w = torch.from_numpy(rs.uniform(-0.3, 0.3, (OUT, 13)).astype(np.float32)).cuda()
    b = torch.from_numpy(rs.uniform(-0.3, 0.3, (OUT,)).astype(np.float32)).cuda()
    offset = [VOXEL[j] / 2 + PC_RANGE[j] for j in range(3)]
    for dist in ('uniform', 'ring'):
        for batch in (1, 4):
            for rows in (60000, 260000):
                pts = make_cloud(rows, batch, dist)
                grid = ops.make_grid(PC_RANGE, VOXEL, GRID, batch)
                hv = lambda: ops.hard_voxelize(pts, grid, PC_RANGE[5], T, MAX_VOXELS)                              # noqa: E731
                res = hv()
                vfe = lambda: ops.pillar_vfe(res.voxels, res.voxel_num_points, res.voxel_coords, VOXEL, offset, w, b)     # noqa: E731

                def both():
                    r = hv()
                    return ops.pillar_vfe(r.voxels, r.voxel_num_points, r.voxel_coords, VOXEL, offset, w, b)

                def both_torch():
                    v, c, n = torch_hard_voxelize(pts, batch)
                    return torch_pillar_vfe(v, n, c, w, b, offset)

                tv, tc, tn = torch_hard_voxelize(pts, batch)
                same = torch.equal(tv, res.voxels) and torch.equal(tc, res.voxel_coords) and torch.equal(tn, res.voxel_num_points)
                err = float((both() - both_torch()).abs().max())
                t = [timed(f) for f in (hv, vfe, both, both_torch)]
                lines.append('%-8s %2d %8d %8d | %s   voxel tensors equal: %s, max |features - torch| %.2g'
                             % (dist, batch, rows * batch, res.voxels.shape[0], ' '.join('%8.3f (%6.3f)' % x for x in t), same, err))
                print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
