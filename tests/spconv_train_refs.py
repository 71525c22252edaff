"""Float64 torch AUTOGRAD over the dense restatement of tests/spconv_refs.py::sparse_conv_ref: the sparse conv scatters its rows into a dense
float64 volume, runs F.conv3d and reads the output sites, so the gradients the training kernels of csrc/spconv3d_train.hip compute are
whatever torch differentiates.  BatchNorm is written out with batch statistics (biased variance for the normalisation, unbiased for the
running update, eps 1e-3, momentum 0.01)."""
import numpy as np
import torch
import torch.nn.functional as F

import spconv_refs as sr

F64 = torch.float64
BN_EPS, BN_MOMENTUM = 1e-3, 0.01


def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=F64)


def sparse_conv_t(x, coords, shape4, weight, bias=None, kernel=3, stride=1, padding=1, out_coords=None):
    """differentiable sparse_conv_ref: x (N, Cin) and weight (Cout, kz, ky, kx, Cin) float64 tensors -> (N_out, Cout) at out_coords (None: the
    input sites, a submanifold layer)"""
    k, s, p = sr.triple(kernel), sr.triple(stride), sr.triple(padding)
    B, D, H, W = shape4
    ci = torch.as_tensor(np.asarray(coords), dtype=torch.int64)
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=F64).index_put((ci[:, 0], ci[:, 1], ci[:, 2], ci[:, 3]), x)
    y = F.conv3d(dense.permute(0, 4, 1, 2, 3), weight.permute(0, 4, 1, 2, 3), stride=s, padding=p)
    oc = ci if out_coords is None else torch.as_tensor(np.asarray(out_coords), dtype=torch.int64)
    out = y.permute(0, 2, 3, 4, 1)[oc[:, 0], oc[:, 1], oc[:, 2], oc[:, 3]]
    return out if bias is None else out + bias


def conv_grads_ref(x, coords, shape4, weight, dy, kernel=3, stride=1, padding=1, out_coords=None):
    """-> dict: dw (Cout, kz, ky, kx, Cin), dx (N, Cin) float64 by autograd of sum(conv(x, W) * dy); dw_abs, dx_abs: the same sums over
    |terms| (the scale of the fp32 summation bound; all factors non-negative, so the gradient IS the sum of absolute terms)"""
    out = {}
    for tag, f in (('', lambda a: a), ('_abs', torch.abs)):
        xt, wt = f(t64(x)).requires_grad_(True), f(t64(weight)).requires_grad_(True)
        y = sparse_conv_t(xt, coords, shape4, wt, None, kernel, stride, padding, out_coords)
        (y * f(t64(dy))).sum().backward()
        out['dw' + tag], out['dx' + tag] = wt.grad.numpy(), xt.grad.numpy()
    return out


def inverse_table_brute(nbr, n_in):
    """inv[k][i] = j where nbr[k][j] == i, else -1"""
    inv = np.full((nbr.shape[0], n_in), -1, np.int32)
    for k in range(nbr.shape[0]):
        for j in range(nbr.shape[1]):
            if nbr[k, j] >= 0:
                assert inv[k, nbr[k, j]] == -1
                inv[k, nbr[k, j]] = j
    return inv


def dw_bound(nbr, dw_abs, cin):
    """(n_terms + 2) 2^-24 sum |terms| per element of dw (Cout, K, Cin): the terms of offset k are the rows with a neighbour there"""
    n = (nbr >= 0).sum(1).astype(np.float64)
    return (n[None, :, None] + 2) * 2.0 ** -24 * dw_abs.reshape(dw_abs.shape[0], -1, cin)


def bn_train_t(y, gamma, beta, rm, rv):
    """batch-statistics BatchNorm of (rows, C); rm / rv (tensors) are replaced by their updated values in the returned tuple"""
    n = y.shape[0]
    mean, var = y.mean(0), y.var(0, unbiased=False)
    out = (y - mean) / torch.sqrt(var + BN_EPS) * gamma + beta
    return out, (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean.detach(), (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var.detach() * n / max(n - 1, 1)


def backbone_train_ref(features, coords, batch_size, sparse_shape, st, last_pad=0, dcanvas=None, condition=None, collect_pre_relu=None):
    """VoxelResBackBone8x under training BatchNorm + HeightCompression on float64.  st: state_dict (numpy).  condition: as
    spconv_refs.backbone_ref (moves the BatchNorm biases IN st so that no pre-ReLU value lies near zero; no gradients then).
    -> dict(spatial_features (B, 128 D, H, W), running {name: array}, grads {param name: array} when dcanvas (B, 128 D, H, W) is given)"""
    P = {k: t64(v).requires_grad_(True) for k, v in st.items() if np.asarray(v).dtype.kind == 'f' and 'running' not in k}
    running = {}
    c = np.asarray(coords)
    shape4 = (batch_size,) + tuple(sparse_shape)

    def bn_relu(y, name, residual=None, relu=True):
        out, running[name + '.running_mean'], running[name + '.running_var'] = bn_train_t(
            y, P[name + '.weight'], P[name + '.bias'], t64(st[name + '.running_mean']), t64(st[name + '.running_var']))
        if residual is not None:
            out = out + residual
        if condition is not None:
            key = name + '.bias'
            old = np.asarray(st[key], np.float64)
            new = (old + condition(out.detach().numpy())).astype(np.float32)
            st[key] = new
            out = out + torch.from_numpy(new.astype(np.float64) - old)
        if collect_pre_relu is not None:
            collect_pre_relu.append(out.detach().numpy().copy())
        return torch.clamp(out, min=0) if relu else out

    def conv(x, c, shape4, name, kernel=3, stride=1, padding=1, out_coords=None):
        return sparse_conv_t(x, c, shape4, P[name + '.weight'], P.get(name + '.bias'), kernel, stride, padding, out_coords)

    def block(x, c, shape4, name):
        y = bn_relu(conv(x, c, shape4, name + '.conv1'), name + '.bn1')
        return bn_relu(conv(y, c, shape4, name + '.conv2'), name + '.bn2', residual=x)

    x = bn_relu(conv(t64(features), c, shape4, 'conv_input.0'), 'conv_input.1')
    x = block(block(x, c, shape4, 'conv1.0'), c, shape4, 'conv1.1')
    for stage, pad in (('conv2', 1), ('conv3', 1), ('conv4', (0, 1, 1))):
        oc = sr.strided_out_coords(c, shape4, 3, 2, pad)
        x = bn_relu(conv(x, c, shape4, stage + '.0.0', 3, 2, pad, oc), stage + '.0.1')
        c, shape4 = oc, (batch_size,) + sr.out_shape(shape4[1:], 3, 2, pad)
        x = block(block(x, c, shape4, stage + '.1'), c, shape4, stage + '.2')
    oc = sr.strided_out_coords(c, shape4, (3, 1, 1), (2, 1, 1), last_pad)
    x = bn_relu(conv(x, c, shape4, 'conv_out.0', (3, 1, 1), (2, 1, 1), last_pad, oc), 'conv_out.1')
    c, shape4 = oc, (batch_size,) + sr.out_shape(shape4[1:], (3, 1, 1), (2, 1, 1), last_pad)
    B, D, H, W = shape4
    ci = torch.as_tensor(c, dtype=torch.int64)
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=F64).index_put((ci[:, 0], ci[:, 1], ci[:, 2], ci[:, 3]), x)
    sf = dense.permute(0, 4, 1, 2, 3).reshape(B, x.shape[1] * D, H, W)                # channel c * D + d
    res = dict(spatial_features=sf.detach().numpy(), running={k: v.numpy() for k, v in running.items()}, rows=len(c))
    if dcanvas is not None:
        (sf * t64(dcanvas)).sum().backward()
        res['grads'] = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()}
    return res


# ---- the seeded case of the whole-backbone training test ---------------------------------------------------------------------------------------
TRAIN_GRID = (24, 32, 32)                   # (z, y, x) voxels: sparse z 25 -> 13 -> 7 -> 3 -> 1
TRAIN_MARGIN = 2e-4                         # no pre-ReLU value of the restatement lies closer to zero than this


def second_train_case(state_shapes, cin=11, batch=2, occupancy=0.02):
    """seeded weights, voxels (mean-VFE order) and a seeded upstream canvas gradient, CONDITIONED under batch-statistics BatchNorm.
    -> st, feats, coords, dcanvas, the reference dict of backbone_train_ref (with grads), the pre-ReLU tensors"""
    rs = np.random.RandomState(21)
    st = {}
    for k, shape in state_shapes.items():
        shape = tuple(shape)
        if len(shape) == 5:
            st[k] = (rs.randn(*shape) * np.sqrt(sr.SECOND_GAIN / (shape[1] * shape[2] * shape[3] * shape[4]))).astype(np.float32)
        elif k.endswith('running_var'):
            st[k] = rs.uniform(0.5, 1.5, shape).astype(np.float32)
        elif k.endswith('num_batches_tracked'):
            st[k] = np.zeros(shape, np.int64)
        elif k.endswith('bn1.weight') or k.endswith('bn2.weight') or k.endswith('.1.weight'):
            st[k] = rs.uniform(0.8, 1.2, shape).astype(np.float32)
        else:
            st[k] = rs.uniform(-0.3, 0.3, shape).astype(np.float32)
    rs = np.random.RandomState(22)
    D, H, W = TRAIN_GRID
    lin = np.flatnonzero(rs.rand(batch * D * H * W) < occupancy)
    b, z, y, x = lin // (D * H * W), (lin // (H * W)) % D, (lin // W) % H, lin % W
    order = np.lexsort((z, y, x, b))
    coords = np.ascontiguousarray(np.stack([b, z, y, x], 1)[order].astype(np.int32))
    feats = rs.uniform(-1.0, 1.0, (len(coords), cin)).astype(np.float32)
    sparse_shape = (D + 1, H, W)
    with torch.no_grad():
        backbone_train_ref(feats, coords, batch, sparse_shape, st, condition=sr.clear_of_zero(1.5 * TRAIN_MARGIN))
    out_sp = (1, H // 8, W // 8)
    dcanvas = rs.uniform(-1.0, 1.0, (batch, 128 * out_sp[0], out_sp[1], out_sp[2])).astype(np.float32)
    pre = []
    want = backbone_train_ref(feats, coords, batch, sparse_shape, st, dcanvas=dcanvas, collect_pre_relu=pre)
    return st, feats, coords, dcanvas, want, pre
