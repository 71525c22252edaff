"""Generates the training fixtures of the SC backbone (SCConvBackbone2dStride4 of the nuScenes PointPillar-Jr models) from the REFERENCE'S
OWN modules (imported read-only through ref_harness).  CPU container only:

    python tests/golden/make_golden_nusc_sc_train.py [block] [backbone]

(a) g22_sc_block_train.npz: the reference's SCBottleneck (workspace/sc_conv.py) in train() mode under autograd, BatchNorm eps 1e-3 /
    momentum 0.01, two cases:
      p32: planes 32 (group width 16, the smallest the 3x3 training kernels take) on (2, 32, 30, 14) -- pooled 7 x 3, neither axis a
           multiple of 4, not square;
      p64: planes 64 on (2, 64, 8, 12) -- pooled 2 x 3, exact multiples.
    Stored: the recipe of the input and of the upstream gradient (pcp_amd.synth.uniform), the weight scheme, and WHOLE the output, the input
    gradient, every parameter gradient and the updated running statistics.
(b) g22_sc_backbone_train.npz: the reference's SCConvBackbone2dStride4 alone, input_channels 16, in train() mode under autograd on a
    seeded (2, 16, 44, 44) canvas (backbone_fixture()): the output and the input gradient whole, every parameter gradient as a digest and
    whole or as 1024 strided values, the updated running statistics (conv_out's BatchNorm with nn.BatchNorm2d's default eps / momentum).

There is no whole-model fixture (pointpillar_jr_nomap under the reference's train step, the fields of g21_nusc_model_train): with the
weights of g20_nusc_mini and the clouds / boxes of make_golden_nusc_train.model_fixture(), none of the seeds 300 .. 399 passed the ReLU-mask
probe, neither on the 60 x 60 mini grid (smallest deviation 1.59e-2 of a tensor's scale) nor on 124 x 124 (2.01e-2), bound 1e-2: a
perturbation of 1e-6 flips ReLU masks somewhere in the 20 conv layers in front of BatchNorms that see 18 .. 98 samples per channel.  The
backbone-level fixture (b) is what pins the layers above the block instead.

Conditioning (reseed until it holds).  Block: no pre-activation of a ReLU within 1e-4 of zero.  Both: the ReLU-mask probe of
make_golden_nusc_train.model_fixture() -- the same step with every weight scaled by 1 + 1e-6 u, u in [-1, 1): no stored gradient moves by more than 1e-2 of its tensor's scale.  The measured
probe deviation goes into the meta.  Fixtures are data; no reference source is stored.
"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(REPO, 'practical-collab-perception_amd'))

import ref_harness as rh  # noqa: E402
from pcp_amd import synth  # noqa: E402

MiB = 1 << 20
BLOCK_CASES = [('p32', 32, (2, 32, 30, 14)), ('p64', 64, (2, 64, 8, 12))]
BLOCK_SCHEME = 'he'
X_STREAM, G_STREAM = 3, 4
RELU_GAP = 1e-4
PROBE_BOUND = 1e-2


def _ref_sc_conv():
    rh.install()
    sys.path.insert(0, os.path.join(rh.REF_ROOT, 'workspace'))
    import sc_conv
    return sc_conv


def _block(sc_conv, planes):
    torch.manual_seed(0)
    blk = sc_conv.SCBottleneck(planes, planes, norm_layer=partial(torch.nn.BatchNorm2d, eps=1e-3, momentum=0.01))
    shapes = {k: [int(x) for x in v.shape] for k, v in blk.state_dict().items()}
    filled = synth.fill_state_dict(shapes, scheme=BLOCK_SCHEME)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return blk.train(), shapes


def _block_step(blk, x_np, g_np, gaps=None):
    """forward + backward; gaps: list that receives min |pre-activation| of every ReLU"""
    hooks = []
    if gaps is not None:
        pre = {}
        for name, mod in (('a', blk.bn1_a), ('b', blk.bn1_b), ('k1', blk.k1[1]), ('k4', blk.scconv.k4[1]), ('bn3', blk.bn3)):
            hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: pre.__setitem__(name, o.detach().clone())))
    x = torch.from_numpy(x_np.copy()).requires_grad_(True)
    blk.zero_grad()
    out = blk(x)
    out.backward(torch.from_numpy(g_np.copy()))
    for h in hooks:
        h.remove()
    if gaps is not None:
        pre['bn3'] = pre['bn3'] + x.detach()                     # relu(bn3(conv3(cat)) + x)
        gaps.extend(float(v.abs().min()) for v in pre.values())
    return out.detach(), x.grad.detach(), {n: p.grad.detach().clone() for n, p in blk.named_parameters()}


def _probe_deviation(base, noisy):
    """largest move of a gradient tensor, as a fraction of that tensor's scale (floor 1e-4 of the largest scale)"""
    gmax = max(float(v.abs().max()) for v in base.values())
    return max((float((noisy[n] - v).abs().max()) / max(float(v.abs().max()), 1e-4 * gmax), n) for n, v in base.items())


def block_fixture():
    sc_conv = _ref_sc_conv()
    out = {}
    cases = {}
    for tag, planes, shape in BLOCK_CASES:
        n = int(np.prod(shape))
        for trial in range(20000):
            seed = synth.SEED_BASE + 2200 + trial
            x_np = synth.uniform(seed, X_STREAM, n, 0.0, 2.0).reshape(shape)                 # a ReLU output feeds every block
            g_np = synth.uniform(seed, G_STREAM, n, -1.0, 1.0).reshape(shape)
            blk, shapes = _block(sc_conv, planes)
            state0 = {k: v.clone() for k, v in blk.state_dict().items()}
            gaps = []
            y, dx, grads = _block_step(blk, x_np, g_np, gaps)
            if min(gaps) < RELU_GAP:
                continue
            stats = {k: v.clone() for k, v in blk.state_dict().items() if 'running_' in k or 'num_batches' in k}
            # the ReLU-mask probe
            blk.load_state_dict(state0)
            with torch.no_grad():
                for i, p_ in enumerate(blk.parameters()):
                    u = torch.from_numpy(synth.uniform(seed, 1000 + i, p_.numel(), -1.0, 1.0).reshape(tuple(p_.shape)))
                    p_.mul_(1.0 + 1e-6 * u)
            _y2, dx2, grads2 = _block_step(blk, x_np, g_np)
            dev, where = _probe_deviation(dict(grads, input=dx), dict(grads2, input=dx2))
            print('%s seed %d: min |ReLU pre-activation| %.3e, probe deviation %.3e at %s' % (tag, seed, min(gaps), dev, where))
            if dev > PROBE_BOUND:
                continue
            break
        else:
            raise RuntimeError('%s: no seed gives a conditioned fixture' % tag)
        cases[tag] = dict(planes=planes, shape=list(shape), seed=seed, x=dict(stream=X_STREAM, lo=0.0, hi=2.0),
                          dout=dict(stream=G_STREAM, lo=-1.0, hi=1.0), state_shapes=shapes, scheme=BLOCK_SCHEME, bn_eps=1e-3, bn_momentum=0.01,
                          min_relu_gap=min(gaps), relu_probe_deviation=dev, param_names=list(grads))
        out[tag + '/out'] = y.numpy()
        out[tag + '/dx'] = dx.numpy()
        for k, v in grads.items():
            out['%s/g/%s' % (tag, k)] = v.numpy()
        for k, v in stats.items():
            out['%s/bn/%s' % (tag, k)] = v.numpy()
        out[tag + '/x_digest'] = np.array([float(x_np.astype(np.float64).sum()), float(np.abs(x_np).max())])
    out['meta_json'] = np.array(json.dumps(dict(cases=cases)))
    path = os.path.join(HERE, 'g22_sc_block_train.npz')
    np.savez_compressed(path, **out)
    print('g22_sc_block_train.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < MiB


BB_IN, BB_FEAT, BB_CANVAS = 16, 64, (2, 16, 44, 44)      # stem 32 x 22 x 22 (pooled 5), main pass 64 x 11 x 11 (pooled 2), out 64 x 11 x 11
BB_SCHEME = 'he'
BB_WHOLE = 4096                                          # gradients up to this many values are stored whole, larger ones as 1024 samples


def _digest(t):
    a = t.detach().double().reshape(-1)
    return np.array([float(a.norm()), float(a.sum()), float(a.abs().max())], dtype=np.float64)


def _sample(t):
    a = t.detach().reshape(-1)
    if a.numel() <= BB_WHOLE:
        return a.numpy().copy()
    return a[::a.numel() // 1024][:1024].numpy().copy()


def backbone_fixture():
    """g22_sc_backbone_train.npz: the reference's SCConvBackbone2dStride4 alone (input_channels 16: stem 32, main pass 64 -- group widths 16
    and 32) in train() mode under autograd, on a seeded (2, 16, 44, 44) canvas with a seeded upstream gradient.  Stem 22 x 22 -> pooled
    5 x 5, main pass 11 x 11 -> pooled 2 x 2: neither side a multiple of 4.  conv_out keeps nn.BatchNorm2d's default eps / momentum.
    Conditioning: the ReLU-mask probe (bound 1e-2, reseeding the canvas).  The block fixture's 1e-4 ReLU gap cannot be asked of 6.4e5 ReLU
    inputs (about 50 of them fall inside it for any seed); the smallest gap is recorded instead."""
    sc_conv = _ref_sc_conv()
    n = int(np.prod(BB_CANVAS))
    oshape = (BB_CANVAS[0], BB_FEAT, BB_CANVAS[2] // 4, BB_CANVAS[3] // 4)
    no = int(np.prod(oshape))

    def build():
        torch.manual_seed(0)
        bb = sc_conv.SCConvBackbone2dStride4(rh.AttrDict(NAME='SCConvBackbone2dStride4', NUM_BEV_FEATURES=BB_FEAT), BB_IN)
        shapes = {k: [int(x) for x in v.shape] for k, v in bb.state_dict().items()}
        filled = synth.fill_state_dict(shapes, scheme=BB_SCHEME)
        bb.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
        return bb.train(), shapes

    def step(bb, x_np, g_np, gaps=None):
        hooks = []
        if gaps is not None:
            for mod in bb.modules():
                if isinstance(mod, torch.nn.ReLU):
                    hooks.append(mod.register_forward_pre_hook(lambda m, i: gaps.append(float(i[0].detach().abs().min()))))
        x = torch.from_numpy(x_np.copy()).requires_grad_(True)
        bb.zero_grad()
        out = bb({'spatial_features': x})['spatial_features_2d']
        out.backward(torch.from_numpy(g_np.copy()))
        for h in hooks:
            h.remove()
        return out.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in bb.named_parameters()}

    for trial in range(100):
        seed = synth.SEED_BASE + 2300 + trial
        x_np = synth.uniform(seed, X_STREAM, n, 0.0, 1.0).reshape(BB_CANVAS)
        g_np = synth.uniform(seed, G_STREAM, no, -1.0, 1.0).reshape(oshape)
        bb, shapes = build()
        gaps = []
        y, dx, grads = step(bb, x_np, g_np, gaps)
        stats = {k: v.clone() for k, v in bb.state_dict().items() if 'running_' in k or 'num_batches' in k}
        pb, _ = build()
        with torch.no_grad():
            for i, p_ in enumerate(pb.parameters()):
                u = torch.from_numpy(synth.uniform(seed, 1000 + i, p_.numel(), -1.0, 1.0).reshape(tuple(p_.shape)))
                p_.mul_(1.0 + 1e-6 * u)
        _y2, dx2, grads2 = step(pb, x_np, g_np)
        dev, where = _probe_deviation(dict(grads, input=dx), dict(grads2, input=dx2))
        print('backbone seed %d: min |ReLU pre-activation| %.3e, probe deviation %.3e at %s' % (seed, min(gaps), dev, where))
        if dev <= PROBE_BOUND:
            break
    else:
        raise RuntimeError('backbone: no seed gives a conditioned fixture')
    names = list(grads)
    meta = dict(cfg=dict(NAME='SCConvBackbone2dStride4', NUM_BEV_FEATURES=BB_FEAT), input_channels=BB_IN, canvas=list(BB_CANVAS), seed=seed,
                x=dict(stream=X_STREAM, lo=0.0, hi=1.0), dout=dict(stream=G_STREAM, lo=-1.0, hi=1.0), state_shapes=shapes, scheme=BB_SCHEME,
                min_relu_gap=min(gaps), relu_probe_deviation=dev, relu_probe_worst_tensor=where, whole_cap=BB_WHOLE, param_names=names)
    out = {'out': y.numpy(), 'dx': dx.numpy(), 'grad_digest': np.stack([_digest(grads[k]) for k in names]),
           'x_digest': np.array([float(x_np.astype(np.float64).sum()), float(np.abs(x_np).max())]), 'meta_json': np.array(json.dumps(meta))}
    for k in names:
        out['g/' + k] = _sample(grads[k])
    for k, v in stats.items():
        out['bn/' + k] = v.numpy()
    path = os.path.join(HERE, 'g22_sc_backbone_train.npz')
    np.savez_compressed(path, **out)
    print('g22_sc_backbone_train.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < MiB


if __name__ == '__main__':
    todo = sys.argv[1:] or ['block', 'backbone']
    torch.set_num_threads(8)
    if 'block' in todo:
        block_fixture()
    if 'backbone' in todo:
        backbone_fixture()
