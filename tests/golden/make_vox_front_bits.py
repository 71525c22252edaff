"""Recorder of the output BITS of the three point-cloud front ends: tests/golden/vox_front_bits.json.

The dynamic pillariser (csrc/voxelize.hip), hard voxelisation (csrc/hard_voxel.hip) and the mean VFE (csrc/spconv3d.hip) share one statement
of the row -> cell arithmetic, the LDS cell-hash aggregation, the run sort and the tile-prefix step (csrc/vox_front.h).  Their other tests
compare each front end with a CPU reference; this file pins every output buffer that is a function of the input alone to the SHA-256 of
its bytes at the commit the JSON names, so a change that claims "same code" is held to it.  tests/test_gpu_vox_front_bits.py runs
`record()` again and demands equality with the committed file.  Every launch runs TWICE and the two hashes must agree.

One seeded cloud serves all cases; `cloud()` asserts on the CPU every condition its docstring names.  What is NOT pinned: the unsorted
bucket order and point_rank, which follow the arrival order of the histogram atomics.

Record with the library of the commit whose bits are to be pinned (PCP_HIP_LIB selects a library built elsewhere):
    PCP_HIP_LIB=<parent build>/libpcp_hip.so python tests/golden/make_vox_front_bits.py --commit <hash of that commit>
"""
import argparse
import ctypes
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
TABLE = os.path.join(HERE, 'vox_front_bits.json')

# 64 x 48 cells of 0.5 m from (0, 0); z from -3 to 2: ten cells of 0.5 m for the mean VFE, one of 5 m for the pillar front ends.  Every
# coordinate is a multiple of 1 / 32, so subtract and divide are exact on x and y
B, NX, NY, NZ = 2, 64, 48, 10
RANGE = [0.0, 0.0, -3.0, 32.0, 24.0, 2.0]
VOXEL = 0.5
NUM_RAW = 4                                     # rows [b, x, y, z, intensity]
T, MAX_VOXELS = 5, 1000                         # hard voxelisation
LONG_PILLAR, SORT_PASS, SORT_TILE = 16, 1024, 2048     # PCP_LONG_PILLAR and the two loops of the long-run sort
HOT = (1, 20, 30, 2500)                         # frame, cx, cy, rows
EXACT = ((0, 3, 3, 1), (0, 5, 40, 16), (1, 60, 7, 17))
MEDIUM_COUNTS = (17, 18, 19, 21, 23, 25, 28, 31, 34, 37, 39, 40)


def _cells_of(pts, nz):
    """float32 cell arithmetic of the reference: (merged pillar id or -1 judged on x and y alone, in range on z too, cz)"""
    f = np.float32
    vz = f((RANGE[5] - RANGE[2]) / nz)
    cx = np.floor((pts[:, 1] - f(RANGE[0])) / f(VOXEL))
    cy = np.floor((pts[:, 2] - f(RANGE[1])) / f(VOXEL))
    cz = np.floor((pts[:, 3] - f(RANGE[2])) / vz)
    ok = (cx >= 0) & (cx < NX) & (cy >= 0) & (cy < NY)
    cell = np.where(ok, pts[:, 0].astype(np.int64) * NX * NY + cx.astype(np.int64) * NY + cy.astype(np.int64), -1)
    return cell, ok & (cz >= 0) & (cz < nz), cz.astype(np.int64)


def cloud():
    """(n, 5) float32 rows [b, x, y, z, intensity], grouped by ascending frame.  Asserted here: two frames; about 6 000 rows, no multiple
    of 1 024; one cell of about 2 500 rows (more than the 2 048-entry tile of the long-run sort, hence also more than its 1 024-element pass),
    interleaved with the other rows of its frame and spread over every cz; a dozen cells of 17 to 40 rows (just above PCP_LONG_PILLAR);
    cells of exactly 1, 16 and 17 rows; rows outside the range on both sides of each axis; frame 0 has more than MAX_VOXELS occupied
    cells and frame 1 fewer; cells of more than T rows."""
    rs = np.random.RandomState(20250917)
    taken = {HOT[:3]} | {e[:3] for e in EXACT}
    free = [(b, cx, cy) for b in range(B) for cx in range(NX) for cy in range(NY) if (b, cx, cy) not in taken]
    pick = [free[i] for i in rs.permutation(len(free))]
    medium = [pick.pop() + (c,) for c in MEDIUM_COUNTS]
    frame0 = [c for c in pick if c[0] == 0][:1400]
    frame1 = [c for c in pick if c[0] == 1][:300]
    filler = [c + (int(rs.randint(1, 4)),) for c in frame0 + frame1]
    rows = []
    for b, cx, cy, count in [HOT] + list(EXACT) + medium + filler:
        for _ in range(count):
            x, y = (cx + rs.randint(1, 16) / 16.0) * VOXEL, (cy + rs.randint(1, 16) / 16.0) * VOXEL
            rows.append([b, x, y, RANGE[2] + rs.randint(0, 160) / 32.0, rs.randint(0, 256) / 256.0])
    n_inside = len(rows)
    for b in range(B):                           # outside the range, both sides of each axis; the z ones sit in cells of the filler
        for axis, values in ((1, (-0.5, -1.0 / 32.0, 32.0, 40.0)), (2, (-7.0, -1.0 / 32.0, 24.0, 24.5)), (3, (-3.0 - 1.0 / 32.0, -9.0, 2.0, 2.5))):
            for v in values:
                _b, cx, cy, _c = [c for c in filler if c[0] == b][rs.randint(300)]
                row = [b, (cx + 0.5) * VOXEL, (cy + 0.5) * VOXEL, -1.0, 0.5]
                row[axis] = v
                rows.append(row)
    pts = np.asarray(rows, np.float32)
    pts = np.concatenate([pts[pts[:, 0] == b][rs.permutation(int((pts[:, 0] == b).sum()))] for b in range(B)])

    n = pts.shape[0]
    assert 5500 <= n <= 6500 and n % 1024 != 0 and (np.diff(pts[:, 0]) >= 0).all() and set(pts[:, 0]) == {0.0, 1.0}
    cell, in_z, cz = _cells_of(pts, NZ)
    _cell1, in_z1, cz1 = _cells_of(pts, 1)
    assert np.array_equal(in_z, in_z1) and (cz1[in_z1] == 0).all()
    assert int(in_z.sum()) == n_inside and int((cell >= 0).sum()) == n_inside + 4 * B
    ids, counts = np.unique(cell[cell >= 0], return_counts=True)
    by_cell = dict(zip(ids.tolist(), counts.tolist()))
    merged = lambda b, cx, cy: b * NX * NY + cx * NY + cy                    # noqa: E731
    hot = merged(*HOT[:3])
    at = np.nonzero(cell == hot)[0]
    assert by_cell[hot] == HOT[3] > SORT_TILE > SORT_PASS and at.max() - at.min() + 1 > 1.1 * HOT[3]
    assert sorted(set(cz[at])) == list(range(NZ)) and in_z[at].all()
    assert sum(1 for c in counts if LONG_PILLAR < c <= 40) >= 12 and all(by_cell[merged(b, x, y)] == c for b, x, y, c in medium)
    assert [by_cell[merged(b, x, y)] for b, x, y, _c in EXACT] == [1, LONG_PILLAR, LONG_PILLAR + 1]
    for axis, lo, hi in ((1, 0.0, 32.0), (2, 0.0, 24.0), (3, -3.0, 2.0)):
        assert (pts[:, axis] < lo).any() and (pts[:, axis] >= hi).any()
    per_frame = [len(set(cell[(pts[:, 0] == b) & in_z])) for b in range(B)]
    assert per_frame[0] > MAX_VOXELS > per_frame[1] > 0, per_frame
    assert (counts > T).sum() > 12
    return pts


def _grid(ops, nz):
    return ops.make_grid(RANGE, [VOXEL, VOXEL, (RANGE[5] - RANGE[2]) / nz], [NX, NY, nz], B)


def _pillariser(got, points):
    from pcp_amd import ops
    grid = _grid(ops, NZ)

    def voxelize():
        vox = ops.voxelize(points, grid, want_inverse=True, want_counts=True)
        ops.voxelize_sort_pillar_rows(vox)
        order = ops.voxelize_row_order(vox)
        P, kept = vox.counters[:2].tolist()
        return {'voxel_coords': vox.voxel_coords[:P], 'unq_inv': vox.unq_inv[:kept], 'unq_cnt': vox.unq_cnt[:P], 'counters': vox.counters,
                'sorted bucket order': order[:kept]}
    got.run('voxelize', voxelize)

    def rows_export():
        vox = ops.pillarise_rows(points, grid, NUM_RAW)
        coords, row_rank, counters, _sr, _sc = ops.pillar_index_export_async(vox)
        return {'coords': coords[:int(counters[0])], 'row_rank': row_rank[:vox.n], 'counters': counters}
    got.run('pillarise_rows + index_export', rows_export)


def _hard_voxel(got, points):
    """the two C entry points called as ops.hard_voxelize calls them, with the whole counter buffer kept"""
    from pcp_amd import lib, ops
    L = lib.load()
    grid = _grid(ops, 1)
    n, stride = points.shape
    assert ops.hard_voxel_nz(grid, RANGE[5]) == 1
    d = points.device

    def launch():
        ws = torch.empty(L.pcp_hard_voxelize_workspace_bytes(ctypes.byref(grid), n), dtype=torch.uint8, device=d)
        coords = torch.empty((n, 4), dtype=torch.int32, device=d)
        num = torch.empty((n,), dtype=torch.int32, device=d)
        counters = torch.empty((ops.HARD_VOXEL_COUNTERS,), dtype=torch.int32, device=d)
        ops.check(L.pcp_hard_voxelize(ops._p(points), n, stride, ctypes.byref(grid), 1, T, MAX_VOXELS, ops._p(ws), ws.numel(), ops._p(coords),
                                      ops._p(num), ops._p(counters), ops._stream()), 'pcp_hard_voxelize')
        host = counters.tolist()
        M, err, per_frame = host[0], host[1], host[4:4 + B]
        assert err == 0 and per_frame[0] == MAX_VOXELS > per_frame[1] > 0 and M == sum(per_frame), (err, per_frame, M)
        voxels = torch.empty((M, T, stride - 1), dtype=torch.float32, device=d)
        ops.check(L.pcp_hard_voxelize_gather(ops._p(points), n, stride, stride - 1, ctypes.byref(grid), T, ops._p(ws), ws.numel(), M, ops._p(num),
                                             ops._p(voxels), ops._stream()), 'pcp_hard_voxelize_gather')
        return {'coords': coords[:M], 'num_points': num[:M], 'voxels': voxels, 'counters': counters}
    got.run('hard_voxelize', launch)


def _mean_vfe(got, points):
    """the two C entry points called as ops.mean_vfe calls them, with the whole counter buffer kept"""
    from pcp_amd import lib, ops
    L = lib.load()
    grid = _grid(ops, NZ)
    n, stride = points.shape
    d = points.device

    def launch():
        ws = torch.empty(L.pcp_mean_vfe_workspace_bytes(ctypes.byref(grid), n), dtype=torch.uint8, device=d)
        coords = torch.empty((n, 4), dtype=torch.int32, device=d)
        counters = torch.empty((ops.MEAN_VFE_COUNTERS,), dtype=torch.int32, device=d)
        ops.check(L.pcp_mean_vfe(ops._p(points), n, stride, ctypes.byref(grid), NZ, ops._p(ws), ws.numel(), ops._p(coords), ops._p(counters),
                                 ops._stream()), 'pcp_mean_vfe')
        M, err = counters[:2].tolist()
        assert err == 0 and M > 0
        feats = torch.empty((M, NUM_RAW), dtype=torch.float32, device=d)
        ops.check(L.pcp_mean_vfe_features(ops._p(points), n, stride, NUM_RAW, ctypes.byref(grid), NZ, ops._p(ws), ws.numel(), M, ops._p(feats),
                                          ops._stream()), 'pcp_mean_vfe_features')
        return {'coords': coords[:M], 'features': feats, 'counters': counters}
    got.run('mean_vfe', launch)


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
    points = torch.from_numpy(cloud()).to(d)
    got = _Table()
    _pillariser(got, points)
    _hard_voxel(got, points)
    _mean_vfe(got, points)
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
