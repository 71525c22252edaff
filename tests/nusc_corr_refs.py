"""Inputs and references of the fused point-head kernel tests (tests/test_gpu_nusc_corr.py): a seeded 8 x 8 map with B = 2, 13-column
points that straddle the map's border and carry rows of a foreign frame (batch index -1), folded MLP / head weights at a given hidden
width, the unfused HIP chain HunterJr runs when the fused kernel is off, and a torch-CPU restatement of the head values."""
import numpy as np
import torch

from pcp_amd import synth

C = 384
B, H, W = 2, 8, 8
MIN_XY = [-3.2, -3.2]
PIX = [0.8, 0.8]
THRESH = 0.3
SEED = synth.SEED_BASE + 2410


def case(hidden, n):
    """numpy inputs: map (B, H, W, C) NHWC, points (n, 13), weights w1 (hidden, C), b1, w2 (C, hidden), b2, wh (8, C), bh"""
    u = lambda stream, count, lo, hi: synth.uniform(SEED + hidden, stream, count, lo, hi)
    bev = u(1, B * H * W * C, 0.0, 1.0).reshape(B, H, W, C)
    pts = u(2, n * 13, -1.0, 1.0).reshape(n, 13)
    pts[:, 1:3] *= 3.6                                        # the map covers +-3.2 m: about one row in five lies outside it
    pts[:, 0] = np.floor(u(3, n, 0.0, 2.0))
    pts[4::7, 0] = -1.0                                       # rows of no frame
    k1, k2 = 1.0 / np.sqrt(C), 1.0 / np.sqrt(hidden)
    w = dict(w1=u(4, hidden * C, -k1, k1).reshape(hidden, C), b1=u(5, hidden, -0.1, 0.1), w2=u(6, C * hidden, -k2, k2).reshape(C, hidden),
             b2=u(7, C, -0.1, 0.1), wh=u(8, 8 * C, -2 * k1, 2 * k1).reshape(8, C), bh=u(9, 8, -0.1, 0.1))
    w['bh'][2] += 0.5                                         # a good share of the rows is dynamic foreground
    return dict(bev=bev, points=pts.astype(np.float32), **{k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()})


def weights_cuda(c):
    return [torch.from_numpy(c[k]).cuda() for k in ('w1', 'b1', 'w2', 'b2', 'wh', 'bh')]


def unfused_chain(c, apply_flow):
    """sample -> two pointwise launches (residual fused into the second) -> heads [-> flow correction -> re-sampling of the corrected rows]:
    the launches of HunterJr.forward with the fused kernel off.  Returns (pf, head8, dyn, points after) as CPU tensors"""
    from pcp_amd import lib, ops, pack
    from pcdet.models.convnet import PackedConv
    bev, pts = torch.from_numpy(c['bev']).cuda(), torch.from_numpy(c['points'].copy()).cuda()
    w1, b1, w2, b2, wh, bh = weights_cuda(c)
    mlp = [PackedConv('plain', w.shape[1], w.shape[0], True, pack.pack_plain(w, b)) for w, b in ((w1, b1), (w2, b2))]
    heads = PackedConv('plain', C, 8, False, pack.pack_plain(wh, bh))
    # rows of no frame are not written by the sampling kernel: they stay the zeros of `out` (the fused kernel writes zeros there)
    pf = ops.bev_sample_bilinear(bev, pts, MIN_XY, PIX, out=torch.zeros((pts.shape[0], C), device='cuda'), channels=C)
    h = pf
    for i, layer in enumerate(mlp):
        h = ops.pointwise(h, layer.w, layer.b, lib.PW_PLAIN, layer.cin, layer.cout, layer.cout_pad, relu=True, residual=pf if i == 1 else None)
    head8 = heads.run(h)
    dyn = None
    if apply_flow:
        dyn = ops.hunter_apply_flow(pts, head8, THRESH)
        ops.bev_sample_bilinear(bev, pts, MIN_XY, PIX, out=pf, row_mask=dyn, channels=C)
    torch.cuda.synchronize()
    return pf.cpu(), head8.cpu(), None if dyn is None else dyn.cpu(), pts.cpu()


def head8_torch(c, pf):
    """the MLP, the residual and the three heads on given sampled rows, torch-CPU float64 rounded to fp32"""
    t = lambda k: torch.from_numpy(c[k]).double()
    f = pf.double()
    h1 = torch.relu(f @ t('w1').t() + t('b1'))
    final = torch.relu(h1 @ t('w2').t() + t('b2')) + f
    return (final @ t('wh').t() + t('bh')).float()


def verdict_margin(head8):
    """how far every row's dynamic-foreground verdict is from flipping: min over rows of |max sigmoid - 0.3| and the top-2 logit gap"""
    p = torch.sigmoid(head8[:, :3].double())
    two = torch.topk(head8[:, :3].double(), 2, dim=1)[0]
    return float(torch.minimum((p.max(1)[0] - THRESH).abs(), two[:, 0] - two[:, 1]).min())
