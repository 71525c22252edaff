"""The slice of spconv's Python surface the SECOND models use, over the HIP kernels of csrc/spconv3d.hip (spconv itself has no ROCm build).
Inference only.  `SparseConvTensor`, `SubMConv3d`, `SparseConv3d` and `SparseSequential` take spconv 2.x's constructor arguments; the conv
weight is shaped (Cout, kz, ky, kx, Cin), the 2.x layout, so a published checkpoint loads by name and shape.

Index tables are cached on the tensor under `indice_key`, as in spconv: every SubMConv3d over the same site set shares one neighbour
table whatever its key (the table is a function of the sites alone), and a SparseConv3d stores its pair under its key.

A `SparseSequential` fuses what the kernel's epilogue can take: conv -> BatchNorm1d (folded into the weights) -> ReLU run as ONE launch.
"""
import torch
import torch.nn as nn

from . import ops, pack


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, table=None, indice_dict=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self._table = table                   # ops.SpconvTable of `indices`, built on first use
        self.indice_dict = indice_dict if indice_dict is not None else {}
        self.trusted_indices = False          # set by a producer that guarantees distinct in-range sites (no read-back to validate)
        # the device-count form (ops.*_dev): `features` / `indices` hold `capacity` rows of which the first *n_dev are real; `dev` is what
        # the layers share over one forward (status words, the replica's buffers, per-level capacities)
        self.n_dev = None
        self.dev = None

    @property
    def capacity(self):
        return int(self.indices.shape[0]) if self.n_dev is not None else None

    def with_device_count(self, n_dev, dev):
        self.n_dev, self.dev = n_dev, dev
        self.trusted_indices = True
        return self

    def replace_feature(self, new_features):
        out = SparseConvTensor(new_features, self.indices, self.spatial_shape, self.batch_size, self._table, self.indice_dict)
        out.trusted_indices = self.trusted_indices
        out.n_dev, out.dev = self.n_dev, self.dev
        return out

    def table(self):
        if self._table is None and self.n_dev is not None:
            self._table = ops.spconv_table_dev(self.indices, self.n_dev, self.batch_size, self.spatial_shape, bufs=self.dev.bufs)
        elif self._table is None:
            idx = self.indices if self.indices.dtype == torch.int32 and self.indices.is_contiguous() else self.indices.int().contiguous()
            self._table = ops.spconv_table(idx, self.batch_size, self.spatial_shape, check_input=not self.trusted_indices)
        return self._table

    # the three steps of a conv layer in this tensor's form; the device-count form names its buffers by dev.level / dev.convs
    def _subm_nbr(self):
        if self.n_dev is None:
            return ops.spconv_build_subm(self.indices, self.table())
        return ops.spconv_build_subm_dev(self.indices, self.table(), self.n_dev, bufs=self.dev.bufs, name='subm%d' % self.dev.level)

    def _strided_index(self, key, kernel_size, stride, padding):
        """-> (out_indices, nbr, out_table, n_out_dev); n_out_dev None in the host-count form"""
        if self.n_dev is None:
            return ops.spconv_build_strided(self.indices, self.table(), kernel_size, stride, padding) + (None,)
        dev = self.dev
        dev.level += 1
        built = ops.spconv_build_strided_dev(self.indices, self.table(), self.n_dev, kernel_size, stride, padding, capacity=dev.capacity_of(dev.level),
                                             status=dev.status, level=dev.level, bufs=dev.bufs, name='strided%d' % dev.level)
        dev.levels.append((str(key), int(built[0].shape[0])))
        return built

    def _conv(self, out_indices, out_spatial_shape, nbr, out_table, n_out_dev, w_packed, bias, residual, relu):
        """the layer's output tensor, in this tensor's form"""
        if self.n_dev is None:
            f = ops.spconv3d(self.features, nbr, w_packed, bias, residual=residual, relu=relu)
        else:
            self.dev.convs += 1
            f = ops.spconv3d_dev(self.features, nbr, n_out_dev, w_packed, bias, residual=residual, relu=relu, bufs=self.dev.bufs,
                                 name='conv%d' % self.dev.convs)
        out = SparseConvTensor(f, out_indices, out_spatial_shape, self.batch_size, out_table, self.indice_dict)
        out.trusted_indices = True
        out.n_dev, out.dev = n_out_dev, self.dev
        return out

    def dense_nhwc(self):
        """(B, H, W, C * D) with channel c * D + d, every element written by one kernel"""
        return ops.spconv_dense(self.features.contiguous(), self.table())

    def dense(self, channels_first=True):
        """(B, C, D, H, W) as spconv's dense() (channels_first False: (B, D, H, W, C))"""
        B, (D, H, W), C = self.batch_size, self.spatial_shape, int(self.features.shape[1])
        x = self.dense_nhwc().view(B, H, W, C, D).permute(0, 3, 4, 1, 2)
        return x if channels_first else x.permute(0, 2, 3, 4, 1)


class DeviceCounts:
    """what the layers of one device-count forward share: the status words the forward's final read examines, the replica's grow-only
    buffers, the optional per-level row capacities (level 0 = the input voxels, level L = the output of the L-th strided layer; None: the
    exact bound) and, filled as the forward goes, the (name, capacity) of every level for the overflow message"""

    def __init__(self, status, bufs=None, row_capacity=None, input_capacity=0):
        self.status, self.bufs = status, bufs
        self.row_capacity = list(row_capacity) if row_capacity is not None else None
        self.level = 0
        self.convs = 0
        self.levels = [('voxels', int(input_capacity))]

    def capacity_of(self, level):
        if self.row_capacity is None or level >= len(self.row_capacity) or self.row_capacity[level] is None:
            return None
        return int(self.row_capacity[level])


class SparseModule(nn.Module):
    pass


def _triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


class SparseConvolution(SparseModule):
    """parameter container + index logic; the arithmetic is ops.spconv3d"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, subm=False,
                 indice_key=None):
        super().__init__()
        if _triple(dilation) != (1, 1, 1) or groups != 1:
            raise NotImplementedError('sparse conv: dilation 1 and groups 1 only')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.subm = bool(subm)
        self.indice_key = indice_key
        if self.subm and self.kernel_size != (3, 3, 3):
            raise NotImplementedError('SubMConv3d: kernel 3 only, got %s' % (self.kernel_size,))
        self.weight = nn.Parameter(torch.empty((self.out_channels,) + self.kernel_size + (self.in_channels,)))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(self.out_channels))
        else:
            self.register_parameter('bias', None)

    def indices_of(self, x):
        """-> (out_indices, out_spatial_shape, nbr, out_table, n_out_dev); n_out_dev None in the host-count form"""
        if self.subm:
            hit = x.indice_dict.get(('subm', id(x.indices)))
            if hit is None or hit[0] is not x.indices:
                hit = (x.indices, x._subm_nbr())
                x.indice_dict[('subm', id(x.indices))] = hit
            return x.indices, x.spatial_shape, hit[1], x.table(), x.n_dev
        key = self.indice_key if self.indice_key is not None else ('anon', id(self))
        hit = x.indice_dict.get(key)
        if hit is None or hit[0] is not x.indices:
            hit = (x.indices,) + x._strided_index(key, self.kernel_size, self.stride, self.padding)
            x.indice_dict[key] = hit
        _, oc, nbr, ot, n_out = hit
        return oc, list(ot.shape4[1:]), nbr, ot, n_out

    def packed_weight(self, bn=None):
        """[K][Cout][cin_pad] weights and (Cout,) bias with `bn` (eval BatchNorm1d) and the conv's own bias folded"""
        w = self.weight.detach()
        if bn is not None:
            w, b = pack.fold_bn(w, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                conv_bias=self.bias.detach() if self.bias is not None else None)
        else:
            b = self.bias.detach().float() if self.bias is not None else torch.zeros(self.out_channels, device=w.device)
        return ops.spconv_pack_weight(w), b.contiguous()

    def run(self, x, w_packed, bias, residual=None, relu=False):
        if not isinstance(x, SparseConvTensor):
            raise TypeError('sparse conv layers take a SparseConvTensor')
        if x.indices.dtype != torch.int32 or not x.indices.is_contiguous():
            x = SparseConvTensor(x.features, x.indices.int().contiguous(), x.spatial_shape, x.batch_size, x._table, x.indice_dict)
        return x._conv(*self.indices_of(x), w_packed, bias, residual, relu)

    def forward(self, x):
        if self.training:
            raise NotImplementedError('inference only')
        w, b = self.packed_weight()
        return self.run(x, w, b)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, subm=True, indice_key=indice_key)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, subm=False, indice_key=indice_key)


class SparseSequential(SparseModule):
    """children named '0', '1', ... like nn.Sequential (the reference's state_dict keys).  Runs conv [+ BatchNorm1d] [+ ReLU] groups as one
    launch each, with the folded weights packed once per eval() (`packed_steps`, dropped by train() / load_state_dict / .to())."""

    def __init__(self, *modules):
        super().__init__()
        for i, m in enumerate(modules):
            self.add_module(str(i), m)
        self._steps = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_packed())

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def invalidate_packed(self):
        for m in self.modules():
            if hasattr(m, '_steps'):
                m._steps = None
            if hasattr(m, '_block_packed'):
                m._block_packed = None

    def _apply(self, fn, *args, **kwargs):
        self._steps = None
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode=True):
        if mode != self.training:
            self._steps = None
        return super().train(mode)

    def packed_steps(self):
        if self._steps is None:
            mods, steps, i = list(self._modules.values()), [], 0
            while i < len(mods):
                m = mods[i]
                if isinstance(m, SparseConvolution):
                    bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d) else None
                    j = i + (2 if bn is not None else 1)
                    relu = j < len(mods) and isinstance(mods[j], nn.ReLU)
                    w, b = m.packed_weight(bn)
                    steps.append(('conv', m, w, b, relu))
                    i = j + (1 if relu else 0)
                elif isinstance(m, (nn.BatchNorm1d, nn.ReLU)):
                    raise NotImplementedError('SparseSequential: %s without a sparse conv in front of it' % type(m).__name__)
                else:
                    steps.append(('module', m))
                    i += 1
            self._steps = steps
        return self._steps

    def forward(self, x):
        if self.training:
            raise NotImplementedError('inference only')
        for st in self.packed_steps():
            x = st[1].run(x, st[2], st[3], relu=st[4]) if st[0] == 'conv' else st[1](x)
        return x
