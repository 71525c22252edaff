"""Times pcp_world_augment_points (csrc/augment.hip) against the same sequence written in eager torch ops on the GPU.

    python bench_augment.py [--iters 30] [--warmup 5] [--out FILE]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_augment.py needs the GPU'
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
