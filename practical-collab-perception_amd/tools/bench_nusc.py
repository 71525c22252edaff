"""Throughput of the nuScenes PointPillar-Jr model (pointpillar_jr_nomap: DynPillarVFE -> scatter -> SCConvBackbone2dStride4 -> CenterHead
with six heads and vel / iou branches) on seeded synthetic 7-column clouds, B = 1 and B = 4, eager model(batch) per step (one host read of
the box counts per step, as in tools/test.py).  Prints a per-layer table of the backbone (B = 4, CUDA events around every launch group)
and, last, one JSON line.

    python practical-collab-perception_amd/tools/bench_nusc.py [--points 260000] [--steps 20] [--warmup 5] [--config nomap|corr_withmap]
                                                                [--unfused-point-head] [--train [--bf16] [--batch 1 4] [--step-timeout 120]]

--config corr_withmap times pointpillar_jr_corr_withmap instead (13-column clouds, HunterJr between the backbone and the head; the corrector
moves points in place, so every step runs on a fresh device copy of the cloud, made inside the timed region); --unfused-point-head runs its
point head as the five-launch chain instead of the fused kernel.

--train (corr_withmap) times TRAINING iterations instead: the synthetic loader's training batch at the real geometry (10-column boxes,
foreground rows, instances_tf), forward + loss.backward() + clipping + the adam_onecycle step, CUDA events, mean of --steps after --warmup;
the per-stage split (CUDA events at the module boundaries of the forward and at the tape entries of the backward) and the peak allocation.
Every step runs under a watchdog of --step-timeout seconds, which ends the process with status 124.  --bf16 selects the bf16 loop.

Synthetic weights (pcp_amd.synth.fill_state_dict, gain 1.6): the arithmetic does not depend on them, only the number of boxes that reach
the NMS does.  A 10-sweep nuScenes cloud holds about 250 000 - 300 000 points.
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

from pcdet.config import EasyDict, cfg_from_yaml_file  # noqa: E402
from pcdet.models import DatasetInfo, build_network  # noqa: E402
from pcp_amd import lib, ops, synth  # noqa: E402
from pcp_amd.conv_dispatch import conv_algo  # noqa: E402

CFGS = os.path.join(HERE, 'cfgs', 'nuscenes_models')


def build_model(config='nomap'):
    cfg = cfg_from_yaml_file(os.path.join(CFGS, 'pointpillar_jr_%s.yaml' % config), EasyDict())
    vs = [p['VOXEL_SIZE'] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
    ds = DatasetInfo(cfg.CLASS_NAMES, cfg.DATA_CONFIG.POINT_CLOUD_RANGE, vs, len(cfg.DATA_CONFIG.POINT_FEATURE_ENCODING.used_feature_list))
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    state = synth.fill_state_dict(shapes, scheme='gain:1.6')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.cuda().eval()


def time_steps(model, pts, batch_size, steps, warmup):
    dev_pts = torch.from_numpy(pts).cuda()
    boxes = 0
    with torch.no_grad():
        for i in range(warmup + steps):
            if i == warmup:
                torch.cuda.synchronize()
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
            pts_in = dev_pts.clone() if getattr(model, 'corrector', None) is not None else dev_pts
            preds, _ = model({'points': pts_in, 'batch_size': batch_size, 'metadata': [{}] * batch_size})
            boxes = sum(int(p['pred_boxes'].shape[0]) for p in preds)
        end.record()
        torch.cuda.synchronize()
    ms = start.elapsed_time(end) / steps
    return ms, boxes


def backbone_table(model, pts, batch_size, reps=10):
    """GPU time per launch group of the backbone, on the canvas of one forward"""
    bd = {'points': torch.from_numpy(pts).cuda(), 'batch_size': batch_size, 'metadata': [{}] * batch_size}
    with torch.no_grad():
        model(bd)
    bb = model.backbone_2d
    pk = bb.packed()
    rows = []

    def timed(name, fn):
        out = fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        rows.append((name, ev[0].elapsed_time(ev[1]) / reps))
        return out

    def block(prefix, blk, x):
        gw = blk.gw
        B, H, W, _ = x.shape
        ab = timed(prefix + 'conv1_a|b 1x1', lambda: blk.conv1.run(x))
        cat = torch.empty((B, H, W, 2 * gw), dtype=torch.float32, device=x.device)
        timed(prefix + 'k1 3x3', lambda: blk.k1.run(ab, out=cat, in_ch_off=0, out_ch_off=0))
        pooled = timed(prefix + 'avgpool (SC)', lambda: ops.avgpool_nhwc(ab, 4, in_ch_off=gw, c=gw))
        s = timed(prefix + 'k2 3x3 @1/4', lambda: blk.k2.run(pooled))
        t = timed(prefix + 'k3 3x3', lambda: blk.k3.run(ab, in_ch_off=gw))
        t0 = t.clone()
        timed(prefix + 'gate (SC)', lambda: ops.sc_gate(t0, ab, s, gw, x_ch_off=gw, out=t))
        timed(prefix + 'k4 3x3', lambda: blk.k4.run(t, out=cat, out_ch_off=gw))
        c3 = blk.conv3
        return timed(prefix + 'conv3 1x1 + residual', lambda: ops.pointwise(cat, c3.w, c3.b, lib.PW_PLAIN, c3.cin, c3.cout, c3.cout_pad,
                                                                                   relu=True, residual=x, residual_before_relu=True))

    with torch.no_grad():
        x = ops.as_nhwc(bd['spatial_features'])
        x = timed('stem.0 3x3 s2', lambda: pk['stem0'].run(x))
        for i, blk in enumerate(pk['stem_blocks']):
            x = block('stem.%d ' % (i + 1), blk, x)
        B, H, W, _ = x.shape
        merged = torch.empty((B, H, W, pk['up'].cout + pk['skip'].cout), dtype=torch.float32, device=x.device)
        timed('conv_skip 1x1', lambda: pk['skip'].run(x, out=merged, out_ch_off=pk['up'].cout))
        y = timed('main_pass.0 3x3 s2', lambda: pk['main0'].run(x))
        for i, blk in enumerate(pk['main_blocks']):
            y = block('main_pass.%d ' % (i + 1), blk, y)
        timed('main_pass.4 convT 2x2', lambda: pk['up'].run(y, out=merged, out_ch_off=0))
        timed('conv_out 3x3 s2', lambda: pk['out'].run(merged))
    return rows


class _Watchdog:
    """ends the process (status 124) when a step takes longer than `seconds`: a hung kernel must not be followed by more launches"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        import threading
        self.t = threading.Timer(self.seconds, lambda: (sys.stderr.write('bench_nusc: a step exceeded %d s\n' % self.seconds), os._exit(124)))
        self.t.daemon = True
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def train_batch(cfg, points, batch_size):
    from pcdet.datasets import build_dataloader
    cfg.DATA_CONFIG.SYNTHETIC.POINTS_PER_FRAME = points
    cfg.DATA_CONFIG.SYNTHETIC.NUM_FRAMES = batch_size
    ds, _loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size, False, training=True)
    return ds.collate_batch([ds[i] for i in range(batch_size)])


def time_train(config, points, batch_size, steps, warmup, step_timeout):
    """ms per training iteration, the per-stage split and the peak allocation of one batch size, on a model of its own"""
    sys.path.insert(0, HERE)
    from train_utils.optimization import build_optimizer, build_scheduler
    cfg = cfg_from_yaml_file(os.path.join(CFGS, 'pointpillar_jr_%s.yaml' % config), EasyDict())
    model = build_model(config)
    batch = train_batch(cfg, points, batch_size)
    ocfg = cfg.OPTIMIZATION
    opt = build_optimizer(model, ocfg)
    sched, _ = build_scheduler(opt, warmup + steps, 1, -1, ocfg)
    dev = {k: torch.from_numpy(batch[k]).cuda() for k in ('points', 'gt_boxes', 'instances_tf')}
    marks = []                                      # (label, event) in launch order of the current step

    def ev(label):
        marks.append((label, torch.cuda.Event(enable_timing=True)))
        marks[-1][1].record()

    def mark_forward(name):
        def hook(_module, _inputs, _output):
            ev('fwd ' + name)                       # returns None: the module's output stays as it is
        return hook
    for name, mod in model.named_children():
        mod.register_forward_hook(mark_forward(name))
    model._pcp_grad_ready_hook = lambda name: ev('bwd ' + name)
    stages, total = {}, 0.0
    torch.cuda.reset_peak_memory_stats()
    model.train()
    for it in range(warmup + steps):
        with _Watchdog(step_timeout):
            del marks[:]
            sched.step(it)
            opt.zero_grad()
            ev('start')
            ret, _tb, _disp = model({'points': dev['points'].clone(), 'gt_boxes': dev['gt_boxes'], 'instances_tf': dev['instances_tf'],
                                     'batch_size': batch_size, 'metadata': batch['metadata']})
            ev('fwd losses')
            model.update_global_step()
            ret['loss'].backward()
            opt.clip_grad_norm(ocfg.GRAD_NORM_CLIP)
            opt.step()
            ev('optimizer')
            torch.cuda.synchronize()
        if it >= warmup:
            for (_l0, e0), (label, e1) in zip(marks[:-1], marks[1:]):
                stages[label] = stages.get(label, 0.0) + e0.elapsed_time(e1) / steps
            total += marks[0][1].elapsed_time(marks[-1][1]) / steps
    return total, stages, torch.cuda.max_memory_allocated(), int(dev['points'].shape[0]), float(ret['loss'].detach())


def main_train(args):
    if args.config != 'corr_withmap':
        raise SystemExit('--train times pointpillar_jr_corr_withmap (--config corr_withmap)')
    if args.bf16:
        os.environ['PCP_CONV_ALGO'] = 'bf16'
    res = {'metric': 'pointpillar_jr_%s training iteration' % args.config, 'points_per_frame': args.points, 'loop': 'bf16' if args.bf16 else 'fp32',
           'cloud': 'synthetic loader, ring, seeded', 'steps': args.steps, 'warmup': args.warmup}
    for B in args.batch:
        ms, stages, peak, n, loss = time_train(args.config, args.points, B, args.steps, args.warmup, args.step_timeout)
        print('B = %d (%d rows), %s loop: %.3f ms per training iteration, peak allocation %.2f GiB, last loss %.4f'
              % (B, n, res['loop'], ms, peak / 2.0 ** 30, loss))
        for label, t in stages.items():
            print('  %-24s %9.3f ms  %5.1f %%' % (label, t, 100.0 * t / ms))
        res['b%d_ms_per_iteration' % B] = round(ms, 3)
        res['b%d_peak_gib' % B] = round(peak / 2.0 ** 30, 3)
        res['b%d_stages_ms' % B] = {k: round(v, 3) for k, v in stages.items()}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=260000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', default='nomap', choices=['nomap', 'corr_withmap'])
    ap.add_argument('--unfused-point-head', action='store_true', help='corr_withmap: the five-launch point head instead of the fused kernel')
    ap.add_argument('--train', action='store_true', help='time training iterations of corr_withmap instead of inference steps')
    ap.add_argument('--bf16', action='store_true', help='--train: the bf16 loop (PCP_CONV_ALGO=bf16)')
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 4], help='--train: the batch sizes to time')
    ap.add_argument('--step-timeout', type=int, default=120, help='--train: seconds one iteration may take before the process is ended')
    args = ap.parse_args()
    if args.train:
        return main_train(args)
    model = build_model(args.config)
    res = {'metric': 'pointpillar_jr_' + args.config, 'points_per_frame': args.points, 'cloud': 'synth.nusc_cloud ring, seeded',
           'conv_algo': conv_algo()}
    corr = getattr(model, 'corrector', None)
    if corr is not None:
        corr.fused_point_head = not args.unfused_point_head
        res['point_head'] = 'fused' if corr.fused_point_head and corr.packed()['fused'] is not None else 'five launches'
    elif args.unfused_point_head:
        ap.error('--unfused-point-head needs a config with a corrector')
    clouds = [synth.nusc_cloud(b, args.points, with_map=args.config != 'nomap', dist='ring') for b in range(4)]
    for B in (1, 4):
        pts = synth.collate(clouds[:B])
        ms, boxes = time_steps(model, pts, B, args.steps, args.warmup)
        res['b%d_ms_per_step' % B] = round(ms, 3)
        res['b%d_frames_per_s' % B] = round(1000.0 * B / ms, 1)
        res['b%d_boxes' % B] = boxes
    rows = backbone_table(model, synth.collate(clouds), 4)
    total = sum(t for _, t in rows)
    sc = sum(t for n, t in rows if '(SC)' in n)
    print('backbone per launch group, B = 4 (ms per step, CUDA events, mean of 10):')
    for n, t in rows:
        print('  %-36s %8.3f  %5.1f %%' % (n, t, 100.0 * t / total))
    print('  %-36s %8.3f' % ('total', total))
    print('  %-36s %8.3f  %5.1f %%' % ('SC-specific kernels (pool, gate)', sc, 100.0 * sc / total))
    res['b4_backbone_ms'] = round(total, 3)
    res['b4_sc_specific_share'] = round(sc / total, 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
