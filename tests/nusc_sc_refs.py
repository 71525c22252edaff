"""Numpy statements for the SC backbone's training kernels (csrc/scconv.hip): torch's nearest source index and the inverse ranges the gate
backward gathers over, and the table of map sizes the kernel tests draw from."""
import numpy as np

# (h, w, sh, sw, r): r is the pool factor that gives sh = h // r (4: the backbone's; 1 and 2: the equal-size and exact-2x cases of nearest_src)
SHAPES = [(30, 14, 7, 3, 4), (15, 15, 3, 3, 4), (8, 12, 2, 3, 4), (4, 4, 1, 1, 4), (7, 5, 1, 1, 4), (7, 3, 7, 3, 1), (6, 14, 3, 7, 2)]


def nearest_src(h, sh):
    """source index of every output index 0 .. h - 1 on one axis: aten/src/ATen/native/UpSample.h nearest_idx with the float32 scale
    (float)sh / h that F.interpolate(size=...) computes -- what pcp_sc_gate does"""
    i = np.arange(h)
    if sh == h:
        return i
    if h == 2 * sh:
        return i >> 1
    scale = np.float32(sh) / np.float32(h)
    return np.minimum(np.floor(i.astype(np.float32) * scale).astype(np.int64), sh - 1)


def inverse_ranges(h, sh):
    """float64 statement: source k is read by the outputs [ceil(k * h / sh), ceil((k + 1) * h / sh)).  Returns (sh, 2) int64."""
    k = np.arange(sh + 1, dtype=np.float64)
    lo = np.ceil(k * np.float64(h) / np.float64(sh)).astype(np.int64)
    return np.stack([lo[:-1], lo[1:]], 1)


def kernel_ranges(h, sh):
    """what nearest_lower of csrc/scconv.hip computes: a float32 guess from the forward's own scale, walked to the exact bound with the
    forward's own index"""
    src = nearest_src(h, sh)
    scale = np.float32(sh) / np.float32(h)

    def lower(k):
        if k >= sh:
            return h
        i = int(np.ceil(np.float32(k) / scale))
        i = min(max(i, 0), h)
        while i > 0 and src[i - 1] >= k:
            i -= 1
        while i < h and src[i] < k:
            i += 1
        return i
    return np.array([[lower(k), lower(k + 1)] for k in range(sh)], dtype=np.int64)


def sc_model_gt(seed, half):
    """(2, 24, 10) in the style of make_golden_nusc_train.model_gt for a +-`half` m range: every head has boxes in frame 0, frame 1 lacks
    heads 3 and 4; padding rows in between; one centre outside the range (clamped)"""
    rs = np.random.RandomState(seed)
    gt = np.zeros((2, 24, 10), dtype=np.float32)
    lim = half - 0.4

    def box(cls):
        return [rs.uniform(-lim, lim), rs.uniform(-lim, lim), rs.uniform(-3, -1), rs.uniform(0.6, 5.0), rs.uniform(0.5, 2.5),
                rs.uniform(0.5, 3.0), rs.uniform(-np.pi, np.pi), rs.uniform(-3, 3), rs.uniform(-3, 3), cls]
    for i, c in enumerate([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 3, 9, 6]):
        gt[0, i + i // 4] = box(c)
    for i, c in enumerate([1, 1, 2, 4, 10, 9, 5]):
        gt[1, 2 * i] = box(c)
    gt[0, 0, 0:2] = [half + 0.5, -half - 0.7]
    return gt
