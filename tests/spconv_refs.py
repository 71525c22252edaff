"""Restatements (numpy / torch-CPU float64) of what the SECOND kernels compute.  spconv and torch_scatter are not installed anywhere the suite
runs, so the oracle is a literal restatement: the mean VFE as mask -> merged id -> np.unique -> float64 mean; a sparse conv as a dense
conv3d on the zero-filled grid kept at the active output sites only; the neighbour table by brute force."""
import numpy as np
import torch
import torch.nn.functional as F


def triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


# ---- mean VFE (dynamic_mean_vfe.py:53-79) ---------------------------------------------------------------------------------------------------
def mean_vfe_ref(points, pc_range, voxel, grid_size, num_features):
    """-> voxel_features float64 (M, C), voxel_coords int32 (M, 4) [b, z, y, x], rows per voxel (M,), mean |x| per voxel float64 (M, C)"""
    pts = points[:, :1 + num_features]
    r = np.asarray(pc_range, np.float32)
    v = np.asarray(voxel, np.float32)
    g = np.asarray(grid_size, np.int64)
    c = np.floor((pts[:, 1:4] - r[:3]) / v).astype(np.int64)                        # float32 subtract and divide
    keep = ((c >= 0) & (c < g)).all(1)
    pts, c = pts[keep], c[keep]
    nx, ny, nz = (int(x) for x in g)
    merged = pts[:, 0].astype(np.int64) * (nx * ny * nz) + c[:, 0] * (ny * nz) + c[:, 1] * nz + c[:, 2]
    unq, inv, cnt = np.unique(merged, return_inverse=True, return_counts=True)
    data = pts[:, 1:].astype(np.float64)
    s = np.zeros((len(unq), num_features))
    a = np.zeros((len(unq), num_features))
    np.add.at(s, inv, data)
    np.add.at(a, inv, np.abs(data))
    coords = np.stack([unq // (nx * ny * nz), unq % nz, (unq % (ny * nz)) // nz, (unq % (nx * ny * nz)) // (ny * nz)], 1).astype(np.int32)
    return s / cnt[:, None], coords, cnt, a / cnt[:, None]


# ---- index tables ----------------------------------------------------------------------------------------------------------------------------
def linear(coords, shape4):
    B, D, H, W = shape4
    c = coords.astype(np.int64)
    return ((c[:, 0] * D + c[:, 1]) * H + c[:, 2]) * W + c[:, 3]


def out_shape(spatial, kernel, stride, padding):
    k, s, p = triple(kernel), triple(stride), triple(padding)
    return tuple((int(spatial[a]) + 2 * p[a] - k[a]) // s[a] + 1 for a in range(3))


def occupancy(coords, shape4):
    occ = np.zeros(shape4, np.float64)
    occ[coords[:, 0], coords[:, 1], coords[:, 2], coords[:, 3]] = 1.0
    return occ


def strided_out_coords(coords, shape4, kernel, stride, padding):
    """active output sites = where a ones-kernel conv of the occupancy is > 0, in ascending linear (b, z, y, x) order"""
    k, s, p = triple(kernel), triple(stride), triple(padding)
    occ = torch.from_numpy(occupancy(coords, shape4))[:, None]
    hit = F.conv3d(occ, torch.ones((1, 1) + k, dtype=torch.float64), stride=s, padding=p)[:, 0].numpy() > 0
    return np.argwhere(hit).astype(np.int32)                                           # argwhere is row-major: ascending linear order


def nbr_brute(in_coords, out_coords, kernel, stride, padding):
    """nbr[d][o] = input row at o * s - p + d (offsets in (kz, ky, kx) ascending order) or -1"""
    k, s, p = triple(kernel), triple(stride), triple(padding)
    where = {tuple(int(x) for x in c): i for i, c in enumerate(in_coords)}
    nbr = np.full((k[0] * k[1] * k[2], len(out_coords)), -1, np.int32)
    for o, (b, z, y, x) in enumerate(out_coords):
        d = 0
        for dz in range(k[0]):
            for dy in range(k[1]):
                for dx in range(k[2]):
                    nbr[d, o] = where.get((int(b), int(z) * s[0] - p[0] + dz, int(y) * s[1] - p[1] + dy, int(x) * s[2] - p[2] + dx), -1)
                    d += 1
    return nbr


def subm_nbr_brute(coords):
    return nbr_brute(coords, coords, 3, 1, 1)


# ---- the convolution -------------------------------------------------------------------------------------------------------------------------
def sparse_conv_ref(features, coords, shape4, weight, bias=None, kernel=3, stride=1, padding=1, subm=True, out_coords=None, with_abs=False):
    """features (N, Cin), weight (Cout, kz, ky, kx, Cin) -> float64 (N_out, Cout) at `out_coords` (the input sites for subm, else the active
    sites of the strided form), and with_abs: sum |w x| per element (the scale of the fp32 dot-product bound)"""
    k, s, p = triple(kernel), triple(stride), triple(padding)
    B, D, H, W = shape4
    cin = features.shape[1]
    dense = torch.zeros((B, cin, D, H, W), dtype=torch.float64)
    f = torch.as_tensor(np.asarray(features), dtype=torch.float64)
    ci = torch.as_tensor(np.asarray(coords), dtype=torch.int64)
    dense[ci[:, 0], :, ci[:, 1], ci[:, 2], ci[:, 3]] = f
    w = torch.as_tensor(np.asarray(weight), dtype=torch.float64).permute(0, 4, 1, 2, 3).contiguous()         # (Cout, Cin, kz, ky, kx)
    y = F.conv3d(dense, w, stride=s, padding=p)
    if out_coords is None:
        out_coords = np.asarray(coords) if subm else strided_out_coords(np.asarray(coords), shape4, k, s, p)
    oc = torch.as_tensor(np.asarray(out_coords), dtype=torch.int64)
    out = y[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]]
    if bias is not None:
        out = out + torch.as_tensor(np.asarray(bias), dtype=torch.float64)
    if not with_abs:
        return out.numpy(), out_coords
    ya = F.conv3d(dense.abs(), w.abs(), stride=s, padding=p)
    return out.numpy(), out_coords, ya[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]].numpy()


def dense_ref(features, coords, shape4):
    """(B, C * D, H, W) with channel c * D + d"""
    B, D, H, W = shape4
    C = features.shape[1]
    out = np.zeros((B, C, D, H, W), features.dtype)
    out[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]] = features
    return out.reshape(B, C * D, H, W)


# ---- the whole backbone in float64 ----------------------------------------------------------------------------------------------------------
def _bn(x, st, pre, eps=1e-3):
    g, b, m, v = (torch.as_tensor(st[pre + n], dtype=torch.float64) for n in ('.weight', '.bias', '.running_mean', '.running_var'))
    return (x - m) / torch.sqrt(v + eps) * g + b


def backbone_ref(features, coords, batch_size, sparse_shape, st, last_pad=0, prefix='', collect_pre_relu=None, condition=None):
    """VoxelResBackBone8x + HeightCompression on float64: st is the state_dict (numpy / tensors).  -> spatial_features (B, 128 * D, H, W).
    collect_pre_relu: a list that receives every pre-ReLU tensor (the conditioning check of the model test).
    condition: a function (rows, C) float64 -> (C,) shift; the BatchNorm bias in front of each ReLU is moved by it IN `st` (rounded to
    float32, the shift applied here is the rounded one), so that a model loaded from `st` afterwards computes what this pass computed."""
    x = torch.as_tensor(np.asarray(features), dtype=torch.float64)
    c = np.asarray(coords)
    shape4 = (batch_size,) + tuple(sparse_shape)

    def relu(t, bn_name):
        if condition is not None:
            key = prefix + bn_name + '.bias'
            old = np.asarray(st[key], np.float64)
            new = (old + condition(t.numpy())).astype(np.float32)
            st[key] = new
            t = t + torch.from_numpy(new.astype(np.float64) - old)
        if collect_pre_relu is not None:
            collect_pre_relu.append(t.numpy().copy())
        return torch.clamp(t, min=0)

    def conv(x, c, shape4, name, subm=True, kernel=3, stride=1, padding=1):
        y, oc = sparse_conv_ref(x.numpy(), c, shape4, st[prefix + name + '.weight'], st.get(prefix + name + '.bias', None), kernel, stride, padding, subm)
        return torch.from_numpy(y), oc

    def block(x, c, shape4, name):
        y, _ = conv(x, c, shape4, name + '.conv1')
        y = relu(_bn(y, st, prefix + name + '.bn1'), name + '.bn1')
        y, _ = conv(y, c, shape4, name + '.conv2')
        return relu(_bn(y, st, prefix + name + '.bn2') + x, name + '.bn2')

    y, _ = conv(x, c, shape4, 'conv_input.0')
    x = relu(_bn(y, st, prefix + 'conv_input.1'), 'conv_input.1')
    x = block(block(x, c, shape4, 'conv1.0'), c, shape4, 'conv1.1')
    for stage, pad in (('conv2', 1), ('conv3', 1), ('conv4', (0, 1, 1))):
        y, c = conv(x, c, shape4, stage + '.0.0', subm=False, stride=2, padding=pad)
        shape4 = (batch_size,) + out_shape(shape4[1:], 3, 2, pad)
        x = relu(_bn(y, st, prefix + stage + '.0.1'), stage + '.0.1')
        x = block(block(x, c, shape4, stage + '.1'), c, shape4, stage + '.2')
    y, c = conv(x, c, shape4, 'conv_out.0', subm=False, kernel=(3, 1, 1), stride=(2, 1, 1), padding=last_pad)
    shape4 = (batch_size,) + out_shape(shape4[1:], (3, 1, 1), (2, 1, 1), last_pad)
    x = relu(_bn(y, st, prefix + 'conv_out.1'), 'conv_out.1')
    return dense_ref(x.numpy(), c, shape4)


# ---- the seeded case of the whole-backbone test ------------------------------------------------------------------------------------------------
SECOND_GRID = (40, 48, 56)                  # (z, y, x) voxels; the backbone's sparse shape is (41, 48, 56)
SECOND_MARGIN = 2e-4                        # no pre-ReLU value of the restatement lies closer to zero than this
SECOND_GAIN = 1.0                           # conv weight variance x fan-in: keeps the maps O(1) through the residual stages


def clear_of_zero(margin):
    """per channel, the smallest shift that leaves no value within `margin` of zero: the gap of width >= 2 margin between neighbouring
    sorted values (or the space beyond either end) whose middle is nearest to zero is moved onto zero.  The ReLU keeps both of its sides."""
    def shift(t):
        out = np.zeros(t.shape[1])
        for ch in range(t.shape[1]):
            s = np.sort(t[:, ch])
            mids = np.concatenate([[s[0] - margin], (s[1:] + s[:-1]) / 2, [s[-1] + margin]])
            ok = np.concatenate([[True], (s[1:] - s[:-1]) >= 2 * margin, [True]])
            cand = mids[ok]
            out[ch] = -cand[np.argmin(np.abs(cand))]
        return out
    return shift


def second_backbone_case(state_shapes, cin=11, batch=2, occupancy=0.012):
    """seeded weights (state_shapes: name -> shape of VoxelResBackBone8x's state_dict), a seeded voxel set in the mean VFE's order and its
    features, CONDITIONED: the BatchNorm biases are moved (clear_of_zero) so that no pre-ReLU value of the float64 restatement lies within
    SECOND_MARGIN of zero.  -> st (numpy, float32 / int64), features, coords, float64 spatial_features, the pre-ReLU tensors"""
    rs = np.random.RandomState(11)
    st = {}
    for k, shape in state_shapes.items():
        shape = tuple(shape)
        if len(shape) == 5:
            st[k] = (rs.randn(*shape) * np.sqrt(SECOND_GAIN / (shape[1] * shape[2] * shape[3] * shape[4]))).astype(np.float32)
        elif k.endswith('running_var'):
            st[k] = rs.uniform(0.5, 1.5, shape).astype(np.float32)
        elif k.endswith('num_batches_tracked'):
            st[k] = np.zeros(shape, np.int64)
        elif k.endswith('bn1.weight') or k.endswith('bn2.weight') or k.endswith('.1.weight'):
            st[k] = rs.uniform(0.8, 1.2, shape).astype(np.float32)
        else:
            st[k] = rs.uniform(-0.3, 0.3, shape).astype(np.float32)
    rs = np.random.RandomState(12)
    D, H, W = SECOND_GRID
    lin = np.flatnonzero(rs.rand(batch * D * H * W) < occupancy)
    b, z, y, x = lin // (D * H * W), (lin // (H * W)) % D, (lin // W) % H, lin % W
    order = np.lexsort((z, y, x, b))                                                   # merged-id order of the mean VFE: (b, x, y, z)
    coords = np.ascontiguousarray(np.stack([b, z, y, x], 1)[order].astype(np.int32))
    feats = rs.uniform(-1.0, 1.0, (len(coords), cin)).astype(np.float32)
    sparse_shape = (D + 1, H, W)
    backbone_ref(feats, coords, batch, sparse_shape, st, condition=clear_of_zero(1.5 * SECOND_MARGIN))       # moves the biases in st
    pre = []
    want = backbone_ref(feats, coords, batch, sparse_shape, st, collect_pre_relu=pre)                        # the plain pass on the final st
    return st, feats, coords, want, pre
