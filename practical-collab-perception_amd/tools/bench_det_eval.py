"""Times the device evaluation (pcp_amd/det_eval.py, csrc/det_eval.hip) beside the float64 numpy restatement of the protocol that the
tests check it against (tests/det_eval_refs.py, plain python loops on the host).

    python bench_det_eval.py [--iters 30] [--warmup 5] [--epoch-frames 1000] [--host-frames 20] [--out FILE]

add():    B = 4 frames x 500 predictions x 40 ground-truth boxes, three classes; DeviceDetectionEval.add() alone (padding with torch ops and
          the match launch; nothing is read back).
result(): an epoch of --epoch-frames such frames (fed in batches of 4 before the clock starts); the two sorts, the curve kernel and the one
          read.
HIP events around every call after a warm-up; mean and min over the timed calls.  The restatement runs once on the add() batch and once on
the first --host-frames frames of the epoch (plain python loops: the epoch figure is quoted per frame)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'tests'))

import det_eval_refs as R  # noqa: E402
from pcp_amd.det_eval import DeviceDetectionEval  # noqa: E402

NAMES = ['car', 'pedestrian', 'bicycle']


def make_frames(n_frames, n_pred=500, n_gt=40, seed=0):
    rng = np.random.RandomState(seed)
    frames = []
    for _ in range(n_frames):
        gt = np.zeros((n_gt, 8), dtype=np.float32)
        gt[:, :2] = rng.uniform(-50, 50, (n_gt, 2))
        gt[:, 2] = -1.0
        gt[:, 3:6] = rng.uniform(0.5, 5.0, (n_gt, 3))
        gt[:, 6] = rng.uniform(-np.pi, np.pi, n_gt)
        gt[:, 7] = 1 + rng.randint(len(NAMES), size=n_gt)
        src = gt[rng.randint(n_gt, size=n_pred)]
        boxes = src[:, :7].copy()
        boxes[:, :2] += rng.normal(0, 1.5, (n_pred, 2)).astype(np.float32)
        boxes[:, 3:6] *= rng.uniform(0.8, 1.25, (n_pred, 3)).astype(np.float32)
        boxes[:, 6] += rng.normal(0, 0.3, n_pred).astype(np.float32)
        frames.append({'boxes': boxes, 'scores': rng.uniform(0.05, 1.0, n_pred).astype(np.float32), 'labels': src[:, 7].astype(np.int64), 'gt': gt})
    return frames


def to_device(frames):
    pds = [{'pred_boxes': torch.from_numpy(f['boxes']).cuda(), 'pred_scores': torch.from_numpy(f['scores']).cuda(),
            'pred_labels': torch.from_numpy(f['labels']).cuda()} for f in frames]
    return pds, torch.from_numpy(np.stack([f['gt'] for f in frames])).cuda()


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.mean(ms)), float(np.min(ms))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--epoch-frames', type=int, default=1000)
    p.add_argument('--host-frames', type=int, default=20)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args()
    lines = ['device: %s' % torch.cuda.get_device_name(0), 'iters %d, warm-up %d' % (args.iters, args.warmup)]

    batch = make_frames(4, seed=1)
    pds, gt = to_device(batch)
    ev = DeviceDetectionEval(NAMES, capacity_frames=4)

    def add():
        ev.reset()
        ev.add(pds, gt)
    mean, best = timed(add, args.warmup, args.iters)
    lines.append('add()    B = 4 x 500 predictions x 40 gt: mean %.3f ms, min %.3f ms per call' % (mean, best))
    t0 = time.perf_counter()
    ref = R.evaluate(batch, NAMES)
    host = (time.perf_counter() - t0) * 1e3
    got = ev.result()[0]
    lines.append('         numpy restatement of the same 4 frames (matching AND curves): %.0f ms; mean_ap device %.6f, restatement %.6f'
                 % (host, got['mean_ap'], ref['mean_ap']))

    epoch = make_frames(args.epoch_frames, seed=2)
    big = DeviceDetectionEval(NAMES, capacity_frames=args.epoch_frames)
    for lo in range(0, args.epoch_frames, 4):
        big.add(*to_device(epoch[lo:lo + 4]))
    torch.cuda.synchronize()
    mean, best = timed(big.result, args.warmup, args.iters)
    lines.append('result() %d-frame epoch (%d records): mean %.3f ms, min %.3f ms per call' % (args.epoch_frames, args.epoch_frames * 500, mean, best))
    sub = epoch[:args.host_frames]
    t0 = time.perf_counter()
    R.evaluate(sub, NAMES)
    host = time.perf_counter() - t0
    lines.append('         numpy restatement of the first %d frames: %.1f s = %.0f ms per frame (x %d frames = %.0f s for the epoch)'
                 % (len(sub), host, host * 1e3 / len(sub), args.epoch_frames, host / len(sub) * args.epoch_frames))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
