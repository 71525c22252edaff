"""Times the SECOND front end and 3D backbone on the device: mean_vfe, the index builds and each of the 21 sparse conv layers of
VoxelResBackBone8x, with their row counts, then the whole v2x_second_ego model.  HIP events around each call, 5 warm-up forwards, mean and
minimum of 30.

    python tools/bench_spconv.py [--out ../../profiles/spconv_bench.txt]

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


def build_model():
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
    ds = SyntheticV2XDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    st = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.cuda().eval()


def make_cloud(batch, dist):
    frames = [np.concatenate([synth.agent_cloud(agent=10 * f + a, n_points=60000, layout='lately', dist=dist) for a in range(6)], 0)
              for f in range(batch)]
    return torch.from_numpy(synth.collate(frames)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
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
