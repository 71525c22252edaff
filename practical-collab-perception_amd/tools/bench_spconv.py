"""Times the SECOND front end and 3D backbone on the device: mean_vfe, the index builds and each of the 21 sparse conv layers of
VoxelResBackBone8x, with their row counts, then the whole v2x_second_ego model.  HIP events around each call, 5 warm-up forwards, mean and
minimum of 30.

    python tools/bench_spconv.py [--out ../../profiles/spconv_bench.txt]
    python tools/bench_spconv.py --train [--out ../../profiles/spconv_train_bench.txt]

    python tools/bench_spconv.py --devcount [--out ../../profiles/spconv_devcount_bench.txt]

--devcount: the whole model on the B = 1 uniform cloud three ways, in alternating rounds -- batch by batch, the device-count form
(MODEL.VFE / BACKBONE_3D.DEVICE_COUNTS) batch by batch, and the device-count form through PipelinedDetector(replicas=2) -- with the peak
allocated bytes of each, then the conv layers of the two forms side by side on the same rows.

--train: one training iteration of the sparse 3D stage (VoxelBackboneTrain + HeightCompression, forward and backward behind a seeded canvas
gradient) on the B = 1 uniform cloud: every conv forward, BatchNorm, weight-gradient and data-gradient call in order, the sums per kind and
the whole iteration (3 warm-up iterations, mean and minimum of 10).

Clouds: the synthetic ego cloud (13 point features, +-52 m), 6 agents x 60 000 rows per frame, B = 1 and 4, uniform and ring.  Grid: the
YAML's 1024 x 1024 x 40 voxels of (0.1, 0.1, 0.2) m.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))

from pcp_amd import ops, synth  # noqa: E402
from pcp_amd import train_ops as tops  # noqa: E402

WARMUP, RUNS = 5, 30
TIMED = ('mean_vfe', 'spconv_table', 'spconv_build_subm', 'spconv_build_strided', 'spconv3d', 'spconv_dense')


class Recorder:
    """wraps the ops entry points the forward goes through; one (name, label, events) record per call, in call order"""

    def __init__(self):
        self.calls, self.orig = [], {}

    def __enter__(self):
        for name in TIMED:
            self.orig[name] = getattr(ops, name)
            setattr(ops, name, self.wrap(name, self.orig[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(ops, name, fn)

    def wrap(self, name, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            label = name
            if name == 'spconv3d':
                label = 'conv %3d -> %3d K=%2d rows %8d -> %8d' % (a[0].shape[1], a[2].shape[1], a[1].shape[0], a[0].shape[0], a[1].shape[1])
            elif name == 'spconv_build_strided':
                label = 'build_strided rows %8d -> %8d' % (a[0].shape[0], out[0].shape[0])
            elif name in ('spconv_build_subm', 'spconv_table'):
                label = '%s rows %8d' % (name[7:], a[0].shape[0])
            elif name == 'mean_vfe':
                label = 'mean_vfe rows %8d -> %8d voxels' % (a[0].shape[0], out[2])
            self.calls.append((label, e0, e1))
            return out
        return timed


def build_model(device_counts=False):
    from pcdet.config import EasyDict, cfg_from_yaml_file
    from pcdet.datasets import SyntheticV2XDataset
    from pcdet.models import build_network
    cwd = os.getcwd()
    os.chdir(HERE)
    try:
        cfg = cfg_from_yaml_file('cfgs/v2x_sim_models/v2x_second_ego.yaml', EasyDict())
    finally:
        os.chdir(cwd)
    cfg.DATA_CONFIG.SYNTHETIC = EasyDict(POINTS_PER_AGENT=1000, NUM_FRAMES=1, DISTRIBUTION='uniform')
    if device_counts:
        cfg.MODEL.VFE.DEVICE_COUNTS = True
        cfg.MODEL.BACKBONE_3D.DEVICE_COUNTS = True
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval()


def make_cloud(batch, dist):
    frames = [np.concatenate([synth.agent_cloud(agent=10 * f + a, n_points=60000, layout='lately', dist=dist) for a in range(6)], 0)
              for f in range(batch)]
    return torch.from_numpy(synth.collate(frames)).cuda()


TRAIN_WARMUP, TRAIN_RUNS = 3, 10
TRAIN_TIMED = ((ops, 'spconv3d', 'conv'), (tops, 'spconv3d_wgrad', 'wgrad'), (tops, 'bn_train_stats', 'bn'), (tops, 'scale_shift_act', 'bn'),
               (tops, 'bn_act_backward', 'bn'), (tops, 'colsum', 'bias'), (tops, 'spconv_invert_nbr', 'tables'), (tops, 'add_relu', 'residual'),
               (tops, 'add_relu_backward', 'residual'), (tops, 'accumulate', 'residual'), (ops, 'spconv_build_subm', 'tables'),
               (ops, 'spconv_build_strided', 'tables'), (ops, 'spconv_table', 'tables'), (ops, 'spconv_dense', 'dense'),
               (tops, 'spconv_dense_backward', 'dense'))


class TrainRecorder:
    """as Recorder, over the entry points one training iteration of the sparse stage goes through; `phase` tells a conv forward from a data
    gradient (both are ops.spconv3d)"""

    def __init__(self):
        self.calls, self.orig, self.phase = [], [], 'forward'

    def __enter__(self):
        for mod, name, kind in TRAIN_TIMED:
            self.orig.append((mod, name, getattr(mod, name)))
            setattr(mod, name, self.wrap(name, kind, getattr(mod, name)))
        return self

    def __exit__(self, *exc):
        for mod, name, fn in self.orig:
            setattr(mod, name, fn)

    def wrap(self, name, kind, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            kd, label = kind, name
            if name == 'spconv3d':
                kd = 'conv forward' if self.phase == 'forward' else 'dgrad'
                label = '%-12s %3d -> %3d K=%2d rows %8d -> %8d' % (kd, a[0].shape[1], a[2].shape[1], a[1].shape[0], a[0].shape[0], a[1].shape[1])
            elif name == 'spconv3d_wgrad':
                label = '%-12s %3d -> %3d K=%2d rows %8d -> %8d' % ('wgrad', a[0].shape[1], a[1].shape[1], a[2].shape[0], a[0].shape[0], a[1].shape[0])
            elif name in ('bn_train_stats', 'scale_shift_act', 'bn_act_backward', 'colsum'):
                label = '%-16s %3d channels, rows %8d' % (name, a[2] if name == 'bn_act_backward' else a[1], a[0].shape[0])
            self.calls.append((kd, label, e0, e1))
            return out
        return timed


def train_main(args):
    from pcdet.models.second_train_path import VoxelBackboneTrain
    from pcp_amd.train_layers import Act
    model = build_model()
    model.backbone_3d.hip_train = True                    # the switch of MODEL.BACKBONE_3D.HIP_TRAIN, set on the built module
    path = VoxelBackboneTrain(model.backbone_3d)
    pts = make_cloud(1, 'uniform')
    with torch.no_grad():
        bd = model.vfe({'points': pts, 'batch_size': 1})
    feats, coords = bd['voxel_features'], bd['voxel_coords']
    dcanvas = None
    per_call, wall = None, []
    with torch.no_grad(), TrainRecorder() as rec:
        for it in range(TRAIN_WARMUP + TRAIN_RUNS):
            rec.calls, rec.phase = [], 'forward'
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = path.forward(feats, coords, 1, trusted=True)
            canvas = out.dense_nhwc()
            if dcanvas is None:
                dcanvas = torch.from_numpy(synth.uniform(7, 1, canvas.numel(), -1.0, 1.0).reshape(tuple(canvas.shape))).cuda()
            rec.phase = 'backward'
            g = tops.spconv_dense_backward(dcanvas, out.indices, (1,) + tuple(out.spatial_shape), int(out.features.shape[1]))
            path.backward(g)
            torch.cuda.synchronize()
            if it >= TRAIN_WARMUP:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms = [(kd, label, e0.elapsed_time(e1)) for kd, label, e0, e1 in rec.calls]
                per_call = per_call or [(kd, label, []) for kd, label, _ in ms]
                for (_, _, acc), (_, _, v) in zip(per_call, ms):
                    acc.append(v)
    lines = ['one training iteration of the sparse 3D stage of v2x_second_ego (VoxelBackboneTrain + HeightCompression, fp32), milliseconds:',
             'mean (min) of %d after %d warm-up iterations, measured on one run; uniform cloud, B = 1, %d rows, %d voxels'
             % (TRAIN_RUNS, TRAIN_WARMUP, pts.shape[0], feats.shape[0]), '']
    sums = {}
    for kd, label, acc in per_call:
        lines.append('  %-64s %8.3f (%7.3f)' % (label, float(np.mean(acc)), float(np.min(acc))))
        sums[kd] = sums.get(kd, 0.0) + float(np.mean(acc))
    lines.append('')
    for kd in ('conv forward', 'bn', 'wgrad', 'dgrad', 'bias', 'residual', 'tables', 'dense'):
        lines.append('  sum %-60s %8.3f' % (kd, sums.get(kd, 0.0)))
    lines.append('  whole iteration of the stage (wall clock, host reads included)    %8.3f (%7.3f)' % (float(np.mean(wall)), float(np.min(wall))))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


DEV_ROUNDS, DEV_BATCHES = 5, 20


def _conv_times(model, pts, name):
    """mean ms of every conv call of one forward form (ops.spconv3d or ops.spconv3d_dev), HIP events, RUNS forwards after WARMUP"""
    acc, orig = None, getattr(ops, name)
    calls = []

    def timed(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(*a, **k)
        e1.record()
        calls.append(('%3d -> %3d K=%2d' % (a[0].shape[1], out.shape[1], a[1].shape[0]), int(a[1].shape[1]), e0, e1))
        return out
    setattr(ops, name, timed)
    try:
        with torch.no_grad():
            for it in range(WARMUP + RUNS):
                del calls[:]
                model({'points': pts, 'batch_size': 1, 'metadata': [{}]})
                torch.cuda.synchronize()
                if it >= WARMUP:
                    acc = acc or [(label, rows, []) for label, rows, _, _ in calls]
                    for (_, _, v), (_, _, e0, e1) in zip(acc, calls):
                        v.append(e0.elapsed_time(e1))
    finally:
        setattr(ops, name, orig)
    return [(label, rows, float(np.mean(v)), float(np.min(v))) for label, rows, v in acc]


def devcount_main(args):
    from pcdet.models.pipelined import PipelinedDetector
    host, dev, dev_p = build_model(False), build_model(True), build_model(True)
    pts = make_cloud(1, 'uniform')
    meta = [{}]
    pipe = PipelinedDetector(dev_p, replicas=2)

    def run_model(model):
        for _ in range(DEV_BATCHES):
            model({'points': pts, 'batch_size': 1, 'metadata': meta})

    def run_pipe():
        for _ in range(DEV_BATCHES):
            pipe.submit(pts, 1, meta)
        pipe.flush()
    modes = [('batch by batch (host counts)', lambda: run_model(host)), ('device counts, batch by batch', lambda: run_model(dev)),
             ('device counts, PipelinedDetector(replicas=2)', run_pipe)]
    ms = {name: [] for name, _ in modes}
    peak = {}
    with torch.no_grad():
        for name, fn in modes:                              # warm-up and peak allocation of each form on its own
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated(), base)
        for _ in range(DEV_ROUNDS):                         # alternating rounds
            for name, fn in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / DEV_BATCHES)
    lines = ['v2x_second_ego, whole model, uniform cloud, B = 1, %d rows: ms per batch (wall clock, host included), %d alternating rounds of %d '
             'batches each' % (pts.shape[0], DEV_ROUNDS, DEV_BATCHES), '']
    for name, _ in modes:
        v = ms[name]
        lines.append('  %-46s mean %7.3f  min %7.3f  max %7.3f   rounds: %s' % (name, np.mean(v), np.min(v), np.max(v), ' '.join('%.3f' % x for x in v)))
    lines.append('')
    lines.append('peak allocated bytes during the form\'s first %d batches (allocated before them: all three models and the cloud)' % DEV_BATCHES)
    for name, _ in modes:
        lines.append('  %-46s peak %14d   above what was allocated before: %14d' % (name, peak[name][0], peak[name][0] - peak[name][1]))
    lines.append('')
    lines.append('conv layers, ms mean (min) of %d forwards: host-count form | device-count form (launch sized by the capacity)' % RUNS)
    h, d = _conv_times(host, pts, 'spconv3d'), _conv_times(dev, pts, 'spconv3d_dev')
    th = td = 0.0
    for (label, rows, hm, hn), (_, cap, dm, dn) in zip(h, d):
        lines.append('  conv %s rows %8d: %7.3f (%7.3f) | capacity %8d: %7.3f (%7.3f)' % (label, rows, hm, hn, cap, dm, dn))
        th, td = th + hm, td + dm
    lines.append('  sum of the 21 convs: %7.3f | %7.3f' % (th, td))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--devcount', action='store_true', help='the whole model three ways: host counts, device counts, device counts pipelined')
    ap.add_argument('--train', action='store_true', help='time one training iteration of the sparse 3D stage instead of the forward')
    args = ap.parse_args()
    if args.train:
        return train_main(args)
    if args.devcount:
        return devcount_main(args)
    model = build_model()
    front = [model.vfe, model.backbone_3d, model.map_to_bev_module]
    lines = ['v2x_second_ego on the device, milliseconds: mean (min) of %d after %d warm-up forwards; 6 agents x 60 000 rows per frame' % (RUNS, WARMUP)]
    for dist in ('uniform', 'ring'):
        for batch in (1, 4):
            pts = make_cloud(batch, dist)
            per_call = None
            with torch.no_grad(), Recorder() as rec:
                for it in range(WARMUP + RUNS):
                    rec.calls = []
                    bd = {'points': pts, 'batch_size': batch}
                    for m in front:
                        bd = m(bd)
                    torch.cuda.synchronize()
                    if it >= WARMUP:
                        ms = [(label, e0.elapsed_time(e1)) for label, e0, e1 in rec.calls]
                        per_call = per_call or [(label, []) for label, _ in ms]
                        for (_, acc), (_, v) in zip(per_call, ms):
                            acc.append(v)
            lines.append('')
            lines.append('%s cloud, B = %d, %d rows' % (dist, batch, pts.shape[0]))
            total = 0.0
            for label, acc in per_call:
                lines.append('  %-52s %8.3f (%7.3f)' % (label, float(np.mean(acc)), float(np.min(acc))))
                total += float(np.mean(acc))
            lines.append('  %-52s %8.3f' % ('sum of the calls above (host reads included)', total))
            with torch.no_grad():
                for _ in range(3):
                    model({'points': pts, 'batch_size': batch, 'metadata': [{}] * batch})
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    model({'points': pts, 'batch_size': batch, 'metadata': [{}] * batch})
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 10
            lines.append('  whole model: %.2f ms per batch, %.1f frames/s' % (dt * 1e3, batch / dt))
            print('\n'.join(lines[-(len(per_call) + 4):]), flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
