"""Plain float64 references (numpy, no GPU) of the small glue kernels, plus the seeded input builders their tests share.

Each function restates one operation of the reference project from its description; the kernel that replaces it is named next to it.

  anchor_decode          anchor_head_template.py:225-272, box_coder_utils.py:46-78, common_utils.limit_period and the sigmoid / max /
                         score mask of the class-agnostic post-processing                      (csrc/anchor.hip, k_anchor_decode)
  apply_flow             hunter_jr.py:259-265                                                  (csrc/hunter.hip, k_apply_flow)
  hunter_meta, local_centroids, object_cat, object_cat_backward, rows_scatter_add
                         hunter_jr.py:165-196 and :50-70                                       (csrc/hunter_train.hip)
  masked_smooth_l1_rows  hunter_jr.py:352-365                                                  (csrc/loss.hip, k_masked_sl1)
  agent_frame_live, zero_maps_unless
                         bev_maker.py:153-190: an agent without a row in the batch has no map  (csrc/voxelize.hip)

Float32 inputs enter the arithmetic as their exact float64 values; nothing here rounds to float32 except where a function says so.
"""
import numpy as np

F32 = np.float32
DIR_OFFSET = F32(0.78539)
DIR_PERIOD = F32(np.pi)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-f64(x)))


def limit_period(val, offset, period):
    """common_utils.limit_period: val - floor(val / period + offset) * period"""
    val = f64(val)
    return val - np.floor(val / float(period) + float(offset)) * float(period)


# ---------------------------------------------------------------------------------------------------------------------
# anchor head
# ---------------------------------------------------------------------------------------------------------------------

def anchor_decode(head, anchors, A, num_class, num_dir_bins, ch_cls, ch_box, ch_dir, dir_offset=DIR_OFFSET, dir_limit_offset=0.0,
                  dir_period=DIR_PERIOD, score_thresh=None):
    """head (B, H, W, ld) float32 NHWC with per location [A x num_class] logits at ch_cls, [A x 7] residuals at ch_box and
    [A x num_dir_bins] direction logits at ch_dir; anchors (H * W * A, 7).  Returns a dict of
      boxes (B, N, 7) float64, cls (B, N, num_class) the input logits, labels (B, N) first maximal class, scores (B, N) float64 sigmoid of
      the maximal logit, mask (B, N) score >= score_thresh (all True without a threshold), dir_bin (B, N) first maximal direction bin,
      floor_arg (B, N) the float64 argument of the floor in limit_period (None without direction bins)."""
    B, H, W, _ = head.shape
    N = H * W * A
    assert anchors.shape == (N, 7)
    px = head.reshape(B, H * W, -1)
    cls = px[:, :, ch_cls:ch_cls + A * num_class].reshape(B, N, num_class)
    enc = f64(px[:, :, ch_box:ch_box + A * 7].reshape(B, N, 7))
    an = f64(anchors)[None]
    diag = np.sqrt(an[..., 3] ** 2 + an[..., 4] ** 2)
    boxes = np.empty((B, N, 7), np.float64)
    boxes[..., 0] = enc[..., 0] * diag + an[..., 0]
    boxes[..., 1] = enc[..., 1] * diag + an[..., 1]
    boxes[..., 2] = enc[..., 2] * an[..., 5] + an[..., 2]
    boxes[..., 3:6] = np.exp(enc[..., 3:6]) * an[..., 3:6]
    rg = enc[..., 6] + an[..., 6]
    dir_bin, floor_arg = None, None
    if num_dir_bins > 0:
        dirp = px[:, :, ch_dir:ch_dir + A * num_dir_bins].reshape(B, N, num_dir_bins)
        dir_bin = np.argmax(dirp, axis=-1)                           # numpy argmax: the first maximal index, like torch.max
        off, per = float(dir_offset), float(dir_period)
        floor_arg = (rg - off) / per + float(dir_limit_offset)
        rg = limit_period(rg - off, dir_limit_offset, per) + off + per * dir_bin
    boxes[..., 6] = rg
    labels = np.argmax(cls, axis=-1)
    scores = sigmoid(np.max(cls, axis=-1))
    mask = np.ones((B, N), bool) if score_thresh is None else scores >= float(score_thresh)
    return dict(boxes=boxes, cls=cls, labels=labels, scores=scores, mask=mask, dir_bin=dir_bin, floor_arg=floor_arg)


def keys_to_scores(keys):
    """the score a non-zero score key stands for: bits(key - 1) as float32; key 0 (masked) gives nan"""
    k = np.asarray(keys).astype(np.int64) & 0xffffffff
    s = (np.maximum(k, 1) - 1).astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(k == 0, np.nan, s)


ANCHOR_SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.62, 1.7]], dtype=np.float32)


def draw_anchor_case(seed, B, H, W, A, num_class, num_dir_bins, ld, ch_cls, ch_box, ch_dir, dir_limit_offset=0.0):
    """Seeded inputs of one anchor-decode case; redraws (seed, seed + 1000, ...) until no anchor's floor argument lies within 1e-4 of an
    integer, so a float32 evaluation cannot take another period than the float64 one.  Returns dict(head, anchors, exact, plant, seed):
      anchors   unequal dx / dy / dz, rotations alternating 0 and pi / 2 along the anchor index
      head      garbage everywhere, then box residuals in +-1, rotation residuals in +-3 pi (several periods), class logits at least
                1e-3 from 0, direction logits N(0, 1) (about half of the anchors choose bin 1)
      planted   (flat anchor indices into B * N, recorded in `plant`)
        exact     rotation-0 anchors whose residual IS dir_offset: val = 0 exactly, the result is dir_offset + period * bin bit for bit;
                  their direction logits choose bin 0 and bin 1 in turn
        cls_tie   every class logit equal (label 0); with three or more classes also a tie of the last two above the first (label 1)
        dir_tie   equal direction logits (bin 0)
        zero      maximal class logit exactly 0 (score exactly 0.5: kept by a >= 0.5 mask)"""
    N = H * W * A
    groups = [(ch_cls, A * num_class), (ch_box, A * 7)] + ([(ch_dir, A * num_dir_bins)] if num_dir_bins else [])
    for i, (s, n) in enumerate(groups):
        assert s >= 0 and s + n <= ld
        for s2, n2 in groups[i + 1:]:
            assert s + n <= s2 or s2 + n2 <= s, 'channel groups overlap'
    for attempt in range(64):
        cur = seed + 1000 * attempt
        rng = np.random.RandomState(cur)
        anchors = np.zeros((H, W, A, 7), np.float32)
        anchors[..., 0] = (np.arange(W, dtype=np.float32) * 0.8 - 0.4 * W)[None, :, None]
        anchors[..., 1] = (np.arange(H, dtype=np.float32) * 0.8 - 0.4 * H)[:, None, None]
        anchors[..., 2] = rng.uniform(-2.0, -0.5, (H, W, A))
        anchors[..., 3:6] = ANCHOR_SIZES[(np.arange(A) // 2) % 3][None, None]
        anchors[..., 6] = np.where(np.arange(A) % 2 == 0, 0.0, np.pi / 2).astype(np.float32)[None, None]
        anchors = anchors.reshape(N, 7)
        head = rng.uniform(-50.0, 50.0, (B, H * W, ld)).astype(np.float32)
        cls = rng.uniform(2e-3, 4.0, (B, N, num_class)) * np.where(rng.rand(B, N, num_class) < 0.5, -1.0, 1.0)
        enc = rng.uniform(-1.0, 1.0, (B, N, 7))
        enc[..., 6] = rng.uniform(-3 * np.pi, 3 * np.pi, (B, N))
        cls, enc = cls.astype(np.float32), enc.astype(np.float32)
        dirp = rng.randn(B, N, max(num_dir_bins, 1)).astype(np.float32)
        # planted anchors: disjoint flat indices, spread over the frames
        idx = rng.permutation(B * N)
        rot0 = [i for i in idx if (i % N) % A % 2 == 0]              # rotation-0 anchors
        plant = dict(exact=np.array(rot0[:4]), cls_tie=idx[8:12], cls_tie_hi=idx[12:16], dir_tie=idx[16:20], zero=idx[20:24])
        plant = {k: np.setdiff1d(v, plant['exact']) if k != 'exact' else v for k, v in plant.items()}
        cf, ef, df = cls.reshape(B * N, -1), enc.reshape(B * N, 7), dirp.reshape(B * N, -1)
        ef[plant['exact'], 6] = DIR_OFFSET
        cf[plant['cls_tie']] = cf[plant['cls_tie'], :1]
        if num_class >= 3:
            cf[plant['cls_tie_hi'], 0] = -1.5
            cf[plant['cls_tie_hi'], 1:] = 0.75
        else:
            plant['cls_tie_hi'] = plant['cls_tie_hi'][:0]
        df[plant['dir_tie']] = df[plant['dir_tie'], :1]
        if num_dir_bins >= 2:                                        # the exact anchors take both bins
            df[plant['exact'], 0] = np.where(np.arange(len(plant['exact'])) % 2 == 0, 1.0, -1.0)
            df[plant['exact'], 1:] = -df[plant['exact'], :1]
        cf[plant['zero']] = -np.abs(cf[plant['zero']])
        cf[plant['zero'], num_class - 1] = 0.0
        head[:, :, ch_cls:ch_cls + A * num_class] = cls.reshape(B, H * W, A * num_class)
        head[:, :, ch_box:ch_box + A * 7] = enc.reshape(B, H * W, A * 7)
        if num_dir_bins:
            head[:, :, ch_dir:ch_dir + A * num_dir_bins] = dirp.reshape(B, H * W, A * num_dir_bins)
        head = head.reshape(B, H, W, ld)
        exact = np.zeros(B * N, bool)
        exact[plant['exact']] = True
        if num_dir_bins == 0:
            break
        x = ((f64(enc[..., 6]) + f64(anchors[None, :, 6]) - float(DIR_OFFSET)) / float(DIR_PERIOD) + float(dir_limit_offset)).reshape(-1)
        if (np.abs(x - np.round(x))[~exact] >= 1e-4).all():
            break
    else:
        raise AssertionError('no seed keeps every anchor 1e-4 away from a period boundary')
    return dict(head=head, anchors=anchors, exact=exact.reshape(B, N), plant=plant, seed=cur)


# ---------------------------------------------------------------------------------------------------------------------
# HunterJr: flow correction, locals / instances, object head glue
# ---------------------------------------------------------------------------------------------------------------------

def apply_flow_mask(head, thresh):
    """hunter_jr.py:259-262: sigmoid of the three class logits, torch.max (first maximal index), dynamic foreground = class 2 with a
    probability above thresh.  Returns (mask bool (n,), p2 float64 (n,))."""
    p = sigmoid(np.asarray(head)[:, :3])
    return (np.argmax(p, axis=1) == 2) & (p[:, 2] > float(F32(thresh))), p[:, 2]


def hunter_meta(points, max_inst, num_sweeps, sweep_col=-2, inst_col=-1):
    """hunter_jr.py:165-196 with numpy.unique.  points (n, C) rows [b, x, y, z, ..., sweep, instance]; foreground is instance > -1.
    Returns dict(fg_idx, fg_local, local_key, local_inst, inst_key, inst_first, inst_last) of int64 arrays."""
    p = np.asarray(points)
    fg_idx = np.nonzero(p[:, inst_col] > -1)[0]
    fg = p[fg_idx]
    key = (fg[:, 0].astype(np.int64) * max_inst + fg[:, inst_col].astype(np.int64)) * num_sweeps + fg[:, sweep_col].astype(np.int64)
    local_key, fg_local = np.unique(key, return_inverse=True)
    inst_key, local_inst = np.unique(local_key // num_sweeps, return_inverse=True)
    n_inst = inst_key.shape[0]
    pos = np.arange(local_key.shape[0])
    # the locals of an instance are contiguous and ascending in sweep
    inst_first = np.full(n_inst, local_key.shape[0], np.int64)
    inst_last = np.full(n_inst, -1, np.int64)
    np.minimum.at(inst_first, local_inst, pos)
    np.maximum.at(inst_last, local_inst, pos)
    return dict(fg_idx=fg_idx, fg_local=fg_local.reshape(-1), local_key=local_key, local_inst=local_inst.reshape(-1), inst_key=inst_key,
                inst_first=inst_first, inst_last=inst_last)


def local_centroids(points, meta):
    """torch_scatter.scatter_mean of the foreground xyz over the locals, and the centred foreground (hunter_jr.py:50-51), float64"""
    xyz = f64(np.asarray(points)[meta['fg_idx'], 1:4])
    n_local = meta['local_key'].shape[0]
    acc = np.zeros((n_local, 3))
    np.add.at(acc, meta['fg_local'], xyz)
    cnt = np.bincount(meta['fg_local'], minlength=n_local).astype(np.float64)
    centroid = acc / cnt[:, None]
    return centroid, xyz - centroid[meta['fg_local']]


def object_cat(lf0, gf, centroid, meta, c, ld_out):
    """hunter_jr.py:61-68: [locals_feat | globals_feat[inst] | centroid | centroid[last-sweep local of inst] | 0 ...]: a gather, float32 kept"""
    inst = meta['local_inst']
    out = np.zeros((lf0.shape[0], ld_out), np.float32)
    out[:, :c] = lf0[:, :c]
    out[:, c:2 * c] = gf[inst][:, :c]
    out[:, 2 * c:2 * c + 3] = centroid
    out[:, 2 * c + 3:2 * c + 6] = centroid[meta['inst_last'][inst]]
    return out


def object_cat_backward(dcat, meta, c):
    """autograd of the concat's first two blocks: dlf0 is the slice (float32), dgf the float64 sum of block 2 over each instance's locals"""
    dlf0 = np.ascontiguousarray(dcat[:, :c])
    dgf = np.zeros((meta['inst_key'].shape[0], c))
    np.add.at(dgf, meta['local_inst'], f64(dcat[:, c:2 * c]))
    return dlf0, dgf


def rows_scatter_add(src, row_index, c, dst):
    """dst[row_index[r], :c] += src[r, :c] for an injective row_index: one float32 addition per element"""
    out = np.array(dst, dtype=np.float32, copy=True)
    out[np.asarray(row_index), :c] = out[np.asarray(row_index), :c] + np.asarray(src, dtype=np.float32)[:, :c]
    return out


def draw_hunter_cloud(seed, B, M, S, n, frac=0.6):
    """random (frame, xyz, ..., sweep, instance) rows as the hunter-meta tests draw them; xyz spread over tens of metres"""
    rng = np.random.RandomState(seed)
    pts = np.zeros((n, 8), np.float32)
    pts[:, 0] = rng.randint(0, B, n)
    pts[:, 1:4] = rng.randn(n, 3) * np.array([20.0, 20.0, 2.0]) + np.array([5.0, -3.0, -1.0])
    pts[:, 4:6] = rng.rand(n, 2)
    pts[:, 6] = rng.randint(0, S, n)
    inst = rng.randint(0, M, n).astype(np.float32)
    inst[rng.rand(n) > frac] = -1.0
    pts[:, 7] = inst
    return pts


def hand_made_hunter_cloud():
    """(B=2, M=4, S=3).  Frame 0: instance 0 seen in sweep 1 only, instance 1 in every sweep, instance 2 with a single point in sweep 0 and
    three in sweep 2, background in between; frame 1: background only.  Returns (points, B, M, S)."""
    rows = []                                  # (frame, sweep, instance, count)
    spec = [(0, 1, 0, 4), (0, 0, -1, 3), (0, 0, 1, 2), (0, 1, 1, 5), (0, 2, 1, 3), (0, 0, 2, 1), (0, 2, -1, 2), (0, 2, 2, 3), (1, 0, -1, 4),
            (1, 2, -1, 3)]
    rng = np.random.RandomState(77)
    for b, sw, inst, cnt in spec:
        for _ in range(cnt):
            rows.append([b, *(rng.randn(3) * 7.0 + 2.0), rng.rand(), rng.rand(), sw, inst])
    pts = np.asarray(rows, dtype=np.float32)
    return pts[rng.permutation(pts.shape[0])], 2, 4, 3


# ---------------------------------------------------------------------------------------------------------------------
# teacher-BEV term
# ---------------------------------------------------------------------------------------------------------------------

def masked_smooth_l1_rows(fused, teacher, c, thresh):
    """hunter_jr.py:357-364: over the rows whose teacher L2 norm is above thresh, the mean of the per-row SUM of smooth-L1 (beta 1) of
    fused - teacher; nan when no row is selected.  fused / teacher (pixels, ld >= c).  Returns (value float64, mask)."""
    f, t = f64(fused)[:, :c], f64(teacher)[:, :c]
    mask = np.sqrt((t * t).sum(1)) > float(F32(thresh))
    d = f - t
    a = np.abs(d)
    row = np.where(a < 1.0, 0.5 * d * d, a - 0.5).sum(1)
    return (float(row[mask].mean()) if mask.any() else float('nan')), mask


def draw_masked_sl1_case(seed, pixels, c, ld_f, ld_t, thresh, all_zero=False):
    """teacher rows are exactly zero (every third row from row 1) or have a norm of at least 2 * thresh (some scaled down to 2.5 * thresh);
    fused - teacher spreads over +-2 with differences of exactly 1.0 and 0.0 planted on multiples of 1/8; the padding holds garbage"""
    rng = np.random.RandomState(seed)
    teacher = (np.round(rng.randn(pixels, ld_t) * 8) / 8).astype(np.float32)
    teacher[:, 0] = 0.5                                                # no accidental all-zero row
    small = np.arange(pixels) % 5 == 2
    scale = f64(2.5 * max(thresh, 1e-3)) / np.sqrt((f64(teacher[:, :c]) ** 2).sum(1))
    teacher[small] = (teacher[small] * scale[small, None]).astype(np.float32)
    zero = np.arange(pixels) % 3 == 1
    if all_zero:
        zero[:] = True
    teacher[zero, :c] = 0.0
    fused = teacher[:, :1].repeat(ld_f, 1)
    fused[:, :min(ld_f, ld_t)] = teacher[:, :min(ld_f, ld_t)]
    d = rng.uniform(-2.0, 2.0, (pixels, ld_f)).astype(np.float32)
    d[:, 1] = 1.0
    d[:, 2] = 0.0
    d[:, 3] = -1.0
    fused = (fused + d).astype(np.float32)
    fused[:, c:] = rng.uniform(-1e3, 1e3, (pixels, ld_f - c)).astype(np.float32)
    teacher[:, c:] = rng.uniform(-1e3, 1e3, (pixels, ld_t - c)).astype(np.float32)
    return fused, teacher, zero


# ---------------------------------------------------------------------------------------------------------------------
# DiscoNet graph path
# ---------------------------------------------------------------------------------------------------------------------

def agent_frame_live(points, col, batch):
    """live[a * batch + b] = 1 iff agent a (0..63) holds a row whose frame index lies in 0..batch-1, the same value for every frame b
    (bev_maker.py:153-170: an agent absent from the batch is skipped, its frames are metadata).  int32 (64 * batch,)"""
    p = np.asarray(points)
    live = np.zeros((64, batch), np.int32)
    if p.shape[0]:
        a, b = p[:, col], p[:, 0]
        ok = (a > -1) & (a < 64) & (b >= 0) & (b < batch)
        live[np.unique(a[ok].astype(np.int64))] = 1
    return live.reshape(-1)


def zero_maps_unless(maps, flag_index, live):
    """map m becomes +0.0 when flag_index[m] >= 0 and live[flag_index[m]] == 0; every other map is left alone"""
    out = np.array(maps, copy=True)
    for m, k in enumerate(flag_index):
        if k >= 0 and live[k] == 0:
            out[m] = 0.0
    return out
