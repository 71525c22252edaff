"""Generates the nuScenes PointPillar-Jr fixtures (tests/golden/g20_nusc*.npz) by running the REFERENCE'S OWN modules (imported
read-only from /root/reference through ref_harness) on seeded synthetic clouds with deterministic weights.  CPU container only:

    python tests/golden/make_golden_nusc.py [mini] [full]

g20_nusc_mini.npz  -- a 60 x 60 grid (range +-6 m): the stem map is 30 x 30 and the main map 15 x 15, so the pooled k2 maps (7 x 7,
                      3 x 3) are NOT a quarter of the map they are interpolated back to (torch's nearest rule, not i // 4).
                      spatial_features_2d and every head map at every pixel for pointpillar_jr_nomap, and the final 9-wide sets of
                      nomap, withmap (12-column cloud) and nomap with CALIB_CLS_SCORE: True.
g20_nusc_full_b4.npz -- the real geometry (512 x 512 grid, 128 x 128 heads), 4 frames: head-map and backbone probes (channel /
                      pixel subsampled) and the exact final set.  The cloud is NOT stored (it would exceed the size limit): the
                      test regenerates it from the recipe in the meta (pcp_amd.synth) and checks its digest.
Weights: synth.fill_state_dict with the smallest gain whose head maps keep an O(1) signal; SCORE_THRESH: the middle of a wide gap of
the candidate scores such that every frame keeps >= 8 boxes and the final sets are invariant under +-1e-4 noise on every head value
(no score within reach of the cut, no IoU within reach of NMS_THRESH).  Fixtures are data; no reference source is stored.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, 'practical-collab-perception_amd'))

import ref_harness as rh  # noqa: E402
from pcp_amd import synth  # noqa: E402

MINI_RANGE = [-6.0, -6.0, -5.0, 6.0, 6.0, 3.0]
NOISE = 1e-4
TRIALS = 6
GAINS = [1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4, 2.6]
MIN_BOXES = 8
IOU_SCALE = 0.1


def load_cfg(yaml_name, overrides=None):
    rh.install()
    from pcdet.config import cfg_from_yaml_file
    cfg = rh.AttrDict()
    cfg_from_yaml_file(os.path.join(rh.REF_ROOT, 'tools', 'cfgs', 'nuscenes_models', yaml_name), cfg)
    for path, val in (overrides or {}).items():
        d = cfg
        keys = path.split('.')
        for k in keys[:-1]:
            d = d[k]
        d[keys[-1]] = val
    return cfg


nusc_cloud = synth.nusc_cloud


def build(yaml_name, scheme, overrides):
    cfg = load_cfg(yaml_name, overrides)
    model, _ds = rh.build_model(cfg)
    sd = model.state_dict()
    shapes = {k: [int(x) for x in v.shape] for k, v in sd.items()}
    filled = synth.fill_state_dict(shapes, scheme=scheme)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return cfg, model, shapes


def forward(model, pts, batch_size):
    bd = {'points': torch.from_numpy(pts.copy()), 'batch_size': batch_size, 'metadata': [{}] * batch_size}
    with torch.no_grad():
        for mod in model.module_list:
            bd = mod(bd)
    pds = [{k: v.detach().clone() for k, v in pd.items()} for pd in model.dense_head.forward_ret_dict['pred_dicts']]
    return bd, pds


def pick_gain(yaml_name, overrides, pts, batch_size):
    for gain in GAINS:
        scheme = 'gain:%g' % gain
        cfg, model, shapes = build(yaml_name, scheme, overrides)
        bd, pds = forward(model, pts, batch_size)
        sd = min(float(pd['hm'].std()) for pd in pds)
        dmax = max(float(pd['dim'].abs().max()) for pd in pds)
        print('  %s gain %.1f: min hm std %.3f, |dim| <= %.2f' % (yaml_name, gain, sd, dmax))
        if 0.15 <= sd and dmax <= 3.5:
            return scheme, cfg, model, shapes, bd, pds
    raise RuntimeError('no gain gives a usable head map')


def _same_set(a_boxes, a_scores, b_boxes, b_scores, tol):
    if a_boxes.shape[0] != b_boxes.shape[0]:
        return False
    used = np.zeros(b_boxes.shape[0], bool)
    for i in range(a_boxes.shape[0]):
        d = np.abs(b_boxes - a_boxes[i])
        d[:, 6] = np.minimum(d[:, 6], np.abs(d[:, 6] - 2 * np.pi)) * (tol / 0.2)
        e = np.maximum(d.max(1), np.abs(b_scores - a_scores[i])) + used * 1e9
        j = int(np.argmin(e))
        if e[j] > tol:
            return False
        used[j] = True
    return True


def _scores(pd, pp):
    s = pd['hm'].sigmoid()
    if pp.get('CALIB_CLS_SCORE', False):
        a = pp.get('CALIB_CLS_SCORE_ALPHA', 0.5)
        s = torch.pow(s, 1.0 - a) * torch.pow(torch.clamp((pd['iou'] + 1) / 2.0, min=0.0, max=1.0), a)
    return s


def robust_threshold(head, batch_size, pds, what):
    pp = head.model_cfg.POST_PROCESSING
    keep = pp.SCORE_THRESH
    K = int(pp.MAX_OBJ_PER_SAMPLE)
    tops = []
    for pd in pds:
        sc = _scores(pd, pp)
        for b in range(batch_size):
            flat = sc[b].reshape(-1)
            tops.append(torch.topk(flat, min(K, flat.numel()))[0].double().numpy())
    union = np.sort(np.concatenate(tops))
    lo, hi = np.quantile(union, 0.5), np.quantile(union, 0.995)
    union = union[(union >= lo) & (union <= hi)]
    gaps = union[1:] - union[:-1]
    gen = torch.Generator().manual_seed(4321)
    try:
        for gi in np.argsort(-gaps)[:40]:
            thr = round(float(union[gi] + union[gi + 1]) / 2.0, 7)
            if gaps[gi] < 5e-5:
                break
            pp.SCORE_THRESH = thr
            with torch.no_grad():
                base = head.generate_predicted_boxes(batch_size, pds)
            counts = [int(d['pred_boxes'].shape[0]) for d in base]
            if min(counts) < MIN_BOXES:
                continue
            ok = True
            for _t in range(TRIALS):
                noisy = [{k: v + (torch.rand(v.shape, generator=gen) * 2 - 1) * NOISE for k, v in pd.items()} for pd in pds]
                with torch.no_grad():
                    got = head.generate_predicted_boxes(batch_size, noisy)
                for a, b in zip(base, got):
                    if not _same_set(a['pred_boxes'].numpy(), a['pred_scores'].numpy(), b['pred_boxes'].numpy(), b['pred_scores'].numpy(),
                                     1e-3):
                        ok = False
                        break
                if not ok:
                    break
            print('  %-8s thr %.7f (gap %.2e) finals %s -> %s' % (what, thr, gaps[gi], counts, 'robust' if ok else 'order-sensitive'))
            if ok:
                return thr, base
    finally:
        pp.SCORE_THRESH = keep
    raise RuntimeError('%s: no threshold gives a perturbation-invariant final set' % what)


def store_finals(out, tag, finals):
    for b, d in enumerate(finals):
        out['%s_boxes_%d' % (tag, b)] = d['pred_boxes'].numpy().copy()
        out['%s_scores_%d' % (tag, b)] = d['pred_scores'].numpy().copy()
        out['%s_labels_%d' % (tag, b)] = d['pred_labels'].numpy().copy()


def meta_of(cfg, yaml_name, layout, shapes, pc_range, scheme, thr):
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = thr
    return dict(model=rh.to_plain(cfg.MODEL), pc_range=pc_range, voxel_size=[0.2, 0.2, 8.0], class_names=list(cfg.CLASS_NAMES),
                yaml=yaml_name, layout=layout, state_shapes=shapes, weight_scheme=scheme)


def mini():
    out, metas = {}, {}
    n = 2000
    pts = synth.collate([nusc_cloud(b, n, 6.1, False) for b in range(2)])
    pts_map = synth.collate([nusc_cloud(b, n, 6.1, True) for b in range(2)])
    # 15 x 15 head maps: the reference's per-class top-K needs MAX_OBJ_PER_SAMPLE <= 225
    ov = {'DATA_CONFIG.POINT_CLOUD_RANGE': MINI_RANGE, 'MODEL.DENSE_HEAD.POST_PROCESSING.MAX_OBJ_PER_SAMPLE': 150}
    scheme, cfg, model, shapes, bd, pds = pick_gain('pointpillar_jr_nomap.yaml', ov, pts, 2)
    out['points'], out['points_map'] = pts, pts_map
    out['spatial_features_2d'] = bd['spatial_features_2d'].numpy()
    for h, pd in enumerate(pds):
        for k, v in pd.items():
            out['head%d_%s' % (h, k)] = v.numpy()
    thr, finals = robust_threshold(model.dense_head, 2, pds, 'nomap')
    store_finals(out, 'nomap', finals)
    metas['nomap'] = meta_of(cfg, 'pointpillar_jr_nomap.yaml', 'nusc', shapes, MINI_RANGE, scheme, thr)
    # CALIB_CLS_SCORE on the same weights and maps
    # the iou branch's last conv is scaled by IOU_SCALE so that (iou + 1) / 2 stays inside (0, 1): at the clamp ends sqrt() turns
    # +-1e-4 into visible score changes and no threshold is robust.  The test applies the same scale (meta 'iou_scale')
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if '.iou.1.' in name:
                prm.mul_(IOU_SCALE)
    _bd, pds_c = forward(model, pts, 2)
    pp = model.dense_head.model_cfg.POST_PROCESSING
    pp.CALIB_CLS_SCORE = True
    thr_c, finals_c = robust_threshold(model.dense_head, 2, pds_c, 'calib')
    store_finals(out, 'calib', finals_c)
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.CALIB_CLS_SCORE = True
    metas['calib'] = meta_of(cfg, 'pointpillar_jr_nomap.yaml', 'nusc', shapes, MINI_RANGE, scheme, thr_c)
    metas['calib']['iou_scale'] = IOU_SCALE
    # withmap: same weight scheme (the state-dict names are those of nomap; only the first PFN layer is wider)
    cfgm, modelm, shapesm = build('pointpillar_jr_withmap.yaml', scheme, ov)
    _bdm, pdsm = forward(modelm, pts_map, 2)
    thr_m, finals_m = robust_threshold(modelm.dense_head, 2, pdsm, 'withmap')
    store_finals(out, 'withmap', finals_m)
    metas['withmap'] = meta_of(cfgm, 'pointpillar_jr_withmap.yaml', 'nusc_map', shapesm, MINI_RANGE, scheme, thr_m)
    # the SCConvBackbone2dStride1 parameter tree (no config of the reference uses it; the build test checks its names and shapes)
    from pcdet.models.backbones_2d import __all__ as bb
    s1 = bb['SCConvBackbone2dStride1'](rh.AttrDict(NAME='SCConvBackbone2dStride1', STEM_CHANNELS=96, NUM_BEV_FEATURES=128), 64)
    metas['stride1'] = dict(cfg=dict(NAME='SCConvBackbone2dStride1', STEM_CHANNELS=96, NUM_BEV_FEATURES=128), input_channels=64,
                            state_shapes={k: [int(x) for x in v.shape] for k, v in s1.state_dict().items()})
    out['meta_json'] = np.array(json.dumps(dict(cases=metas, noise=NOISE, trials=TRIALS)))
    path = os.path.join(HERE, 'g20_nusc_mini.npz')
    np.savez_compressed(path, **out)
    print('mini:', os.path.getsize(path), 'bytes; finals', {t: [out['%s_boxes_%d' % (t, b)].shape[0] for b in range(2)]
                                                           for t in ('nomap', 'calib', 'withmap')})


FULL_POINTS = 40000
FULL_PROBE_PIX = 8          # every 8th row / column of the 128 x 128 maps
FULL_PROBE_SF_CH = 24       # every 24th channel of spatial_features_2d


def full_cloud():
    return synth.collate([nusc_cloud(b, FULL_POINTS, 52.0, False) for b in range(4)])


def full():
    out = {}
    pts = full_cloud()
    scheme, cfg, model, shapes, bd, pds = pick_gain('pointpillar_jr_nomap.yaml', {}, pts, 4)
    sf = bd['spatial_features_2d'].numpy()
    out['sf_probe'] = sf[:, ::FULL_PROBE_SF_CH, ::FULL_PROBE_PIX, ::FULL_PROBE_PIX].copy()
    for h, pd in enumerate(pds):
        for k, v in pd.items():
            out['head%d_%s_probe' % (h, k)] = v.numpy()[:, :, ::FULL_PROBE_PIX, ::FULL_PROBE_PIX].copy()
    thr, finals = robust_threshold(model.dense_head, 4, pds, 'full')
    store_finals(out, 'nomap', finals)
    meta = meta_of(cfg, 'pointpillar_jr_nomap.yaml', 'nusc', shapes, list(cfg.DATA_CONFIG.POINT_CLOUD_RANGE), scheme, thr)
    meta.update(cloud=dict(frames=4, points_per_frame=FULL_POINTS, xy_half=52.0, first_agent=40, z_range=[-5.0, 3.0]),
                points_sha256=hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest(), probe_pix=FULL_PROBE_PIX,
                probe_sf_ch=FULL_PROBE_SF_CH)
    out['meta_json'] = np.array(json.dumps(dict(cases=dict(nomap=meta), noise=NOISE, trials=TRIALS)))
    path = os.path.join(HERE, 'g20_nusc_full_b4.npz')
    np.savez_compressed(path, **out)
    print('full:', os.path.getsize(path), 'bytes; finals', [out['nomap_boxes_%d' % b].shape[0] for b in range(4)])


if __name__ == '__main__':
    which = sys.argv[1:] or ['mini', 'full']
    torch.set_num_threads(os.cpu_count() or 1)
    if 'mini' in which:
        mini()
    if 'full' in which:
        full()
