"""Generates tests/golden/g23_vfe_train_widths.npz: the REFERENCE'S OWN DynamicPillarVFE (imported read-only through ref_harness, as
g16_pfn_variants does) in train() mode under autograd on the CPU, at raw widths the training PillarFeatureNet had no kernel for.  CPU
container only:

    python tests/golden/make_golden_nusc_vfe_train.py

Cases (USE_ABSLOTE_XYZ, no WITH_DISTANCE, USE_NORM, NUM_FILTERS [64, 64]; BatchNorm1d eps 1e-3 / momentum 0.01, the reference's own):
    w10: 10 raw columns, F = 16 -- the width pointpillar_jr_withmap reads; the 16-float feature row needs no padding
    w7:   7 raw columns, F = 13 -- padded to 16
    w12: 12 raw columns, F = 18 -- padded to 32
Cloud: the grid of g16 (range +-12.8 m, z -8 .. 0, 0.2 m voxels: 128 x 128), 2 frames of 700 points of the 13-column 'lately' layout cut to
1 + num_raw columns, plus the crowded cells of test_vfe_train_forward_backward_matches_autograd (17, 16, 40, 300, 1500 and 33 points in one
cell each), rows shuffled.  Upstream gradient: dL/d pillar_features = synth.uniform(seed, G_STREAM, P * 64, -1, 1).

Stored per case: the points, voxel_coords, pillar_features, the updated running statistics (and num_batches_tracked), every parameter
gradient; in the meta the seeds, the weight scheme, the gradient recipe and the measured conditioning margins.

Conditioning (the cloud is reseeded until both hold; the measured values go into the meta):
  * relu_gap >= 1e-4: for both PFN layers, no (pillar, channel) whose LARGEST pre-activation (the BatchNorm output of the row that wins the
    pillar max; when every row is negative, the row nearest to winning) is within 1e-4 of zero -- a ReLU mask that decides a routed gradient
    is never an fp32 coin toss;
  * top2_gap >= 1e-5: no (pillar, channel) whose two largest post-ReLU values are closer than 1e-5 unless both are exactly 0 -- arg-max
    routing is never an fp32 coin toss;
  * the six crowded cells hold exactly their 16, 17, 33, 40, 300 and 1500 rows (no point of the base cloud fell into one).
Recorded but not asked for: the smallest |pre-activation| of layer 0 over ALL rows (every row's own activation feeds the second Linear).
The file holds data only; no reference source is stored.
"""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, 'practical-collab-perception_amd'))

import ref_harness as rh  # noqa: E402
from pcp_amd import synth  # noqa: E402

MiB = 1 << 20
PC_RANGE = [-12.8, -12.8, -8.0, 12.8, 12.8, 0.0]          # MINI_RANGE of make_golden.py (g16)
VOXEL = [0.2, 0.2, 8.0]
CASES = [('w10', 10), ('w7', 7), ('w12', 12)]
CROWDED = (17, 16, 40, 300, 1500, 33)
SCHEME = 'he'
G_STREAM = 4
RELU_GAP = 1e-4
TOP2_GAP = 1e-5
MAX_TRIALS = 2000000


def cloud(seed, num_raw):
    """2 x 700 points of the 'lately' layout + the crowded cells, shuffled, cut to 1 + num_raw columns"""
    base = synth.collate([synth.agent_cloud(agent=10 + b, n_points=700, layout='lately', seed=seed, xy_half=13.1) for b in range(2)])
    rs = np.random.RandomState(seed % (1 << 31))
    x_lo, y_lo = PC_RANGE[0], PC_RANGE[1]
    extra = []
    for i, k in enumerate(CROWDED):
        q = np.zeros((k, base.shape[1]), np.float32)
        q[:, 0] = i % 2
        q[:, 1] = x_lo + 0.2 * (20 + 3 * i) + rs.uniform(0.01, 0.19, k)
        q[:, 2] = y_lo + 0.2 * (31 + i) + rs.uniform(0.01, 0.19, k)
        q[:, 3] = rs.uniform(-6.0, -1.0, k)
        q[:, 4:] = base[rs.randint(0, base.shape[0], k), 4:]
        extra.append(q)
    pts = np.concatenate([base] + extra, 0)
    pts = pts[rs.permutation(pts.shape[0])]
    return np.ascontiguousarray(pts[:, :1 + num_raw])


def _segment_top2(v, inv, n):
    """per (segment, channel): the largest value and the second largest (-inf for a segment of one row)"""
    idx = inv.view(-1, 1).expand_as(v)
    top = torch.full((n, v.shape[1]), -np.inf, dtype=v.dtype).scatter_reduce(0, idx, v, 'amax', include_self=True)
    pos = torch.arange(v.shape[0]).view(-1, 1).expand_as(v)
    big = v.shape[0]
    first = torch.full(top.shape, big, dtype=torch.long).scatter_reduce(0, idx, torch.where(v == top[inv], pos, big), 'amin', include_self=True)
    rest = torch.where(pos == first[inv], torch.full_like(v, -np.inf), v)
    second = torch.full((n, v.shape[1]), -np.inf, dtype=v.dtype).scatter_reduce(0, idx, rest, 'amax', include_self=True)
    return top, second


def margins(pre, inv):
    """pre: the two BatchNorm outputs (N, 32), (N, 64); inv (N,) pillar of each row -> (relu_gap, top2_gap, layer-0 gap over all rows)"""
    n = int(inv.max()) + 1
    relu_gap, top2_gap = np.inf, np.inf
    for v in pre:
        top, _ = _segment_top2(v, inv, n)
        relu_gap = min(relu_gap, float(top.abs().min()))
        a, b = _segment_top2(torch.relu(v), inv, n)
        d = torch.where((b == -np.inf) | ((a == 0) & (b == 0)), torch.full_like(a, np.inf), a - b)
        top2_gap = min(top2_gap, float(d.min()))
    return relu_gap, top2_gap, float(pre[0].abs().min())


def build(vfe_cls, num_raw, grid):
    mc = rh.AttrDict(NAME='DynPillarVFE', WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, USE_NORM=True, NUM_FILTERS=[64, 64])
    vfe = vfe_cls(model_cfg=mc, num_point_features=num_raw, voxel_size=VOXEL, grid_size=grid, point_cloud_range=np.asarray(PC_RANGE, np.float32))
    shapes = {'vfe.' + k: [int(x) for x in v.shape] for k, v in vfe.state_dict().items()}
    filled = synth.fill_state_dict(shapes, scheme=SCHEME)
    vfe.load_state_dict({k[len('vfe.'):]: torch.from_numpy(v) for k, v in filled.items()})
    for layer in vfe.pfn_layers:
        assert layer.norm.eps == 1e-3 and layer.norm.momentum == 0.01
    return vfe.train(), shapes


def run(vfe, pts, grad_seed=None):
    """one train-mode forward (and, with grad_seed, the backward of sum(pillar_features * R)); returns the batch dict, the BatchNorm outputs
    and the row -> pillar map the module used"""
    seen = {}
    hooks = [vfe.pfn_layers[0].register_forward_pre_hook(lambda m, i: seen.__setitem__('inv', i[1].detach().clone()))]
    for li, layer in enumerate(vfe.pfn_layers):
        hooks.append(layer.norm.register_forward_hook(lambda m, i, o, li=li: seen.__setitem__(li, o.detach().clone())))
    vfe.zero_grad()
    with torch.set_grad_enabled(grad_seed is not None):
        bd = vfe({'points': torch.from_numpy(pts.copy()), 'batch_size': 2})
        if grad_seed is not None:
            pf = bd['pillar_features']
            R = torch.from_numpy(synth.uniform(grad_seed, G_STREAM, pf.numel(), -1.0, 1.0).reshape(tuple(pf.shape)))
            (pf * R).sum().backward()
    for h in hooks:
        h.remove()
    return bd, [seen[0], seen[1]], seen['inv']


def _ref_vfe():
    rh.install()
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE
    assert rh.REF_ROOT in sys.modules[DynamicPillarVFE.__module__].__file__
    rng_pc = np.asarray(PC_RANGE, dtype=np.float32)
    grid = np.round((rng_pc[3:] - rng_pc[:3]) / np.asarray(VOXEL, dtype=np.float32)).astype(np.int64)
    return DynamicPillarVFE, grid


def search(ci):
    """the first seed of case `ci` whose cloud is conditioned -> (seed, trials, relu_gap, top2_gap, layer-0 gap over all rows)"""
    torch.set_num_threads(1)
    DynamicPillarVFE, grid = _ref_vfe()
    tag, nr = CASES[ci]
    t0 = time.time()
    best = -1.0
    for trial in range(MAX_TRIALS):
        seed = synth.SEED_BASE + 23000000 + 2000000 * ci + trial
        vfe, _shapes = build(DynamicPillarVFE, nr, grid)
        _bd, pre, inv = run(vfe, cloud(seed, nr))
        relu_gap, top2_gap, all_rows_gap = margins(pre, inv)
        score = min(relu_gap / RELU_GAP, top2_gap / TOP2_GAP)
        if score > best:
            best = score
            print('%s trial %d (%.0f s): relu gap %.3e, top-2 gap %.3e' % (tag, trial, time.time() - t0, relu_gap, top2_gap), flush=True)
        # the crowded cells keep their sizes (no point of the base cloud fell into one): 16 and 17 rows sit on either side of PCP_LONG_PILLAR
        exact = sorted(torch.bincount(inv).tolist())[-len(CROWDED):] == sorted(CROWDED)
        if relu_gap >= RELU_GAP and top2_gap >= TOP2_GAP and exact:
            return seed, trial + 1, relu_gap, top2_gap, all_rows_gap
    raise RuntimeError('%s: no seed gives a conditioned fixture' % tag)


def main():
    import multiprocessing as mp
    with mp.get_context('spawn').Pool(len(CASES)) as pool:               # the three searches side by side, one thread each
        found = pool.map(search, range(len(CASES)))
    DynamicPillarVFE, grid = _ref_vfe()
    out, cases = {}, {}
    for (tag, nr), (seed, trials, relu_gap, top2_gap, all_rows_gap) in zip(CASES, found):
        pts = cloud(seed, nr)
        vfe, shapes = build(DynamicPillarVFE, nr, grid)
        bd, pre, inv = run(vfe, pts, grad_seed=seed)
        assert margins(pre, inv)[:2] == (relu_gap, top2_gap)
        P = int(bd['voxel_coords'].shape[0])
        counts = torch.bincount(inv, minlength=P)
        names = [n for n, _p in vfe.named_parameters()]
        assert len(names) == 6 and tuple(vfe.pfn_layers[0].linear.weight.shape) == (32, nr + 6)
        cases[tag] = dict(num_raw=nr, F=nr + 6, seed=seed, trials=trials, state_shapes=shapes, scheme=SCHEME, bn_eps=1e-3, bn_momentum=0.01,
                          dpillar=dict(seed=seed, stream=G_STREAM, lo=-1.0, hi=1.0), relu_gap=relu_gap, top2_gap=top2_gap,
                          layer0_all_rows_relu_gap=all_rows_gap, pillars=P, rows=int(inv.shape[0]), longest_pillars=sorted(counts.tolist())[-7:],
                          param_names=names)
        out[tag + '/points'] = pts
        out[tag + '/voxel_coords'] = bd['voxel_coords'].numpy().astype(np.int32)
        out[tag + '/pillar_features'] = bd['pillar_features'].detach().numpy()
        for n, p_ in vfe.named_parameters():
            out['%s/g/%s' % (tag, n)] = p_.grad.numpy().copy()
        for k, v in vfe.state_dict().items():
            if 'running_' in k or 'num_batches' in k:
                out['%s/bn/%s' % (tag, k)] = v.numpy().copy()
        print('%s: seed %d after %d trials, P = %d, rows = %d, longest pillars %s' % (tag, seed, trials, P, inv.shape[0],
                                                                                    cases[tag]['longest_pillars']), flush=True)
    out['meta_json'] = np.array(json.dumps(dict(cases=cases, pc_range=PC_RANGE, voxel_size=VOXEL, grid_size=[int(g) for g in grid],
                                                relu_gap_bound=RELU_GAP, top2_gap_bound=TOP2_GAP)))
    path = os.path.join(HERE, 'g23_vfe_train_widths.npz')
    np.savez_compressed(path, **out)
    print('g23_vfe_train_widths.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < MiB


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
