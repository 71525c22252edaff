"""Inputs and references of the fused point-head kernel at a given channel count (tests/test_gpu_second_corr.py and
tests/test_second_corr_cpu.py): what tests/nusc_corr_refs.py provides at its fixed C = 384, with the width as an argument.  A seeded 8 x 8
map with B = 2, 13-column points of which about one row in five lies outside the map and the rows 4::7 belong to no frame (batch index -1),
folded MLP / head weights, the unfused HIP chain HunterJr runs when the fused kernel is off, and the sampled rows by the oracle's CPU
sampler.  The width-free helpers (head8_torch, verdict_margin) are nusc_corr_refs's own."""
import numpy as np
import torch

from nusc_corr_refs import head8_torch, verdict_margin  # noqa: F401  (re-exported)
from pcp_amd import synth

B, H, W = 2, 8, 8
MIN_XY = [-3.2, -3.2]
PIX = [0.8, 0.8]
THRESH = 0.3
# the seed is chosen on the float64 restatement alone (tests/test_second_corr_cpu.py): every (hidden, n) case of the GPU test keeps its
# dynamic-foreground verdicts more than 1e-3 from flipping, and at n >= 31 the dynamic share lies strictly between 0 and 1
SEED = synth.SEED_BASE + 2560
HIDDEN = (32, 64)
NS = (1, 31, 32, 33, 97)


def case(channels, hidden, n):
    """numpy inputs: map (B, H, W, channels) NHWC, points (n, 13), weights w1 (hidden, channels), b1, w2 (channels, hidden), b2,
    wh (8, channels), bh"""
    C = channels
    u = lambda stream, count, lo, hi: synth.uniform(SEED + C + hidden, stream, count, lo, hi)
    bev = u(1, B * H * W * C, 0.0, 1.0).reshape(B, H, W, C)
    pts = u(2, n * 13, -1.0, 1.0).reshape(n, 13)
    pts[:, 1:3] *= 3.6                                        # the map covers +-3.2 m: about one row in five lies outside it
    pts[:, 0] = np.floor(u(3, n, 0.0, 2.0))
    pts[4::7, 0] = -1.0                                       # rows of no frame
    k1, k2 = 1.0 / np.sqrt(C), 1.0 / np.sqrt(hidden)
    w = dict(w1=u(4, hidden * C, -k1, k1).reshape(hidden, C), b1=u(5, hidden, -0.1, 0.1), w2=u(6, C * hidden, -k2, k2).reshape(C, hidden),
             b2=u(7, C, -0.1, 0.1), wh=u(8, 8 * C, -2 * k1, 2 * k1).reshape(8, C), bh=u(9, 8, -0.1, 0.1))
    w['bh'][2] += 0.5                                         # a good share of the rows is dynamic foreground
    return dict(bev=np.ascontiguousarray(bev, dtype=np.float32), points=pts.astype(np.float32),
                **{k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()})


def weights_cuda(c):
    return [torch.from_numpy(c[k]).cuda() for k in ('w1', 'b1', 'w2', 'b2', 'wh', 'bh')]


def oracle_pf(c):
    """the sampled rows (n, C) by oracle/bev.py's CPU sampler (fp32 torch); rows of no frame are 0"""
    from oracle import bev as obev
    bev = torch.from_numpy(c['bev']).permute(0, 3, 1, 2).contiguous()
    pf, _coord = obev.sample_point_features(bev, torch.from_numpy(c['points']), MIN_XY, PIX)
    return pf


def dynamic_rows(head8):
    """the dynamic-foreground verdict of hunter_jr.py:257-262 on given head values"""
    p = torch.sigmoid(head8[:, :3].double())
    return (p.argmax(1) == 2) & (p.max(1)[0] > THRESH)


def unfused_chain(c, apply_flow):
    """sample -> two pointwise launches (residual fused into the second) -> heads [-> flow correction -> re-sampling of the corrected rows]:
    the launches of HunterJr.forward with the fused kernel off, at the width of the case.  Returns (pf, head8, dyn, points after) as CPU
    tensors"""
    from pcp_amd import lib, ops, pack
    from pcdet.models.convnet import PackedConv
    C = c['bev'].shape[3]
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
