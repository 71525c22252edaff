"""Train-mode execution of VoxelResBackBone8x (the SECOND family's sparse 3D stage), forward AND backward, on the HIP kernels of
csrc/spconv3d.hip and csrc/spconv3d_train.hip.  Opt-in: MODEL.BACKBONE_3D.HIP_TRAIN (and MODEL.VFE.HIP_TRAIN for the parameter-free
DynMeanVFE in front of it); without the switch the modules refuse train() as before.

Like train_path.BackboneTrain for BaseBEVBackbone, `VoxelBackboneTrain` is an object of its own that reads the modules' parameters; the spconv
modules' own forward keeps refusing training mode.  No torch.autograd inside.  One layer:

  forward   raw conv  ops.spconv3d with the unfolded weight and the conv's own bias (zeros where it has none)
            bn        tops.bn_train_stats on (rows, C) (batch statistics, running statistics updated), tl.bump_batches_tracked,
                      tops.scale_shift_act (normalise [+ ReLU])
  backward  bn+relu   tops.bn_act_backward in place on the incoming gradient (BatchNorm parameter gradients)
            bias      tops.colsum of the pre-BN gradient (the blocks' convs; mathematically zero under batch statistics, computed all the same)
            wgrad     tops.spconv3d_wgrad into weight.grad, the parameter's own (Cout, kz, ky, kx, Cin)
            dgrad     ops.spconv3d again: a submanifold layer on its own table with mirrored transposed weights, a strided layer on the inverse
                      table (tops.spconv_invert_nbr) with transposed weights.  conv_input has none: the voxel means carry no gradient.

SparseBasicBlock is relu(bn2(conv2(relu(bn1(conv1 x)))) + x): the SC backbone's add-ReLU helpers on (rows, C); the gradient of the block input
is always the masked residual gradient first, conv1's data gradient added to it.

Weights are packed once per optimizer step (tl.StepClock).  Index tables live on the SparseConvTensor as in inference: one neighbour table per
stage, one inverse table per strided layer, built once per forward.  The stage is fp32 in the bf16 loop as well.  A layer with no rows launches
nothing and leaves zero gradients.
"""
import torch

from pcp_amd import ops, spconv
from pcp_amd import train_layers as tl
from pcp_amd import train_ops as tops
from pcp_amd.train_layers import ensure_grad


def _empty(shape, dev, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=dev)


class _SpConvBN:
    """one sparse conv + BatchNorm1d under batch statistics [+ ReLU]"""

    def __init__(self, conv, bn, relu, need_dx, name):
        self.conv, self.bn, self.relu, self.need_dx, self.name = conv, bn, relu, need_dx, name
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.vec = None
        self.saved = None
        self._step = -1

    def _weights(self):
        if self._step == tl.StepClock.step:
            return self._w
        w = self.conv.weight.detach()
        dev = w.device
        b = self.conv.bias.detach().float().contiguous() if self.conv.bias is not None else torch.zeros(self.cout, dtype=torch.float32, device=dev)
        self._w = dict(fw=ops.spconv_pack_weight(w), fb=b)
        if self.need_dx:
            self._w.update(bw=ops.spconv_pack_weight_dgrad(w, mirror=self.conv.subm), bb=torch.zeros(self.cin, dtype=torch.float32, device=dev))
        self._step = tl.StepClock.step
        return self._w

    def forward(self, x):
        """x: SparseConvTensor.  Returns the SparseConvTensor of relu?(bn(conv(x)))."""
        conv, bn = self.conv, self.bn
        n_in = int(x.features.shape[0])
        dev = x.features.device
        if n_in == 0:                                              # no rows: no table either
            osp = list(x.spatial_shape) if conv.subm else list(ops.spconv_out_shape(x.spatial_shape, conv.kernel_size, conv.stride, conv.padding))
            oc, nbr, ot = _empty((0, 4), dev, torch.int32), None, None
        else:
            oc, osp, nbr, ot = conv.indices_of(x)[:4]
        n_out = int(oc.shape[0])
        if n_out == 0:
            self.saved = None
            self.n_in = n_in
            out = _empty((0, self.cout), dev)
        else:
            w = self._weights()
            y = ops.spconv3d(x.features, nbr, w['fw'], w['fb'], relu=False)
            self.vec = tops.bn_train_stats(y, self.cout, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean,
                                           bn.running_var, vec=self.vec)
            tl.bump_batches_tracked(bn)
            out = _empty((n_out, self.cout), dev)
            tops.scale_shift_act(y, self.cout, self.vec, self.relu, out)
            # the table of the data gradient: a submanifold layer's own (symmetric under mirroring the offset), a strided layer's inverse
            back = None
            if self.need_dx:
                back = nbr if conv.subm else tops.spconv_invert_nbr(nbr, n_in)
            self.saved = (x.features, y, nbr, back)
        t = spconv.SparseConvTensor(out, oc, osp, x.batch_size, ot, x.indice_dict)
        t.trusted_indices = True
        return t

    def _zero_grads(self):
        for p in (self.conv.weight, self.conv.bias, self.bn.weight, self.bn.bias):
            if p is not None:
                ensure_grad(p).zero_()

    def backward(self, dout):
        """dout: (n_out, cout) float32, a buffer of its own (overwritten).  Returns (n_in, cin) or None."""
        if self.saved is None:
            self._zero_grads()
            return torch.zeros((self.n_in, self.cin), dtype=torch.float32, device=self.conv.weight.device) if self.need_dx else None
        x, y, nbr, back = self.saved
        tops.bn_act_backward(dout, y, self.cout, self.vec, self.relu, ensure_grad(self.bn.weight), ensure_grad(self.bn.bias))
        if self.conv.bias is not None:
            tops.colsum(dout, self.cout, ensure_grad(self.conv.bias))
        tops.spconv3d_wgrad(x, dout, nbr, ensure_grad(self.conv.weight))
        if not self.need_dx:
            return None
        w = self._weights()
        return ops.spconv3d(dout, back, w['bw'], w['bb'], relu=False)


class _SpBlockTrain:
    """SparseBasicBlock: relu(bn2(conv2(relu(bn1(conv1 x)))) + x)"""

    def __init__(self, blk, name):
        self.c = blk.conv1.out_channels
        self.conv1 = _SpConvBN(blk.conv1, blk.bn1, True, True, name + '.conv1')
        self.conv2 = _SpConvBN(blk.conv2, blk.bn2, False, True, name + '.conv2')
        self.out = None

    def forward(self, x):
        z = self.conv2.forward(self.conv1.forward(x))
        if z.features.shape[0]:
            tops.add_relu(z.features, x.features, self.c)                     # in place over bn2's output
        self.out = z.features
        return z

    def backward(self, dout):
        """dout: (rows, c), overwritten.  Returns the gradient of the block input: the masked residual gradient, then conv1's data gradient."""
        if not self.out.shape[0]:
            self.conv2.backward(dout)
            self.conv1.backward(dout)
            return dout
        dres = torch.empty_like(dout)
        tops.add_relu_backward(dout, self.out, self.c, dz2=dres)
        g = self.conv1.backward(self.conv2.backward(dout))
        tops.accumulate(dres, g, self.c)
        return dres


class VoxelBackboneTrain:
    """conv_input -> conv1 .. conv4 -> conv_out of VoxelResBackBone8x, layer by layer"""

    def __init__(self, bb):
        self.m = bb
        self.layers = [_SpConvBN(bb.conv_input[0], bb.conv_input[1], True, False, 'conv_input')]
        self.stage_ends = []                  # index in self.layers of the last layer of conv1 .. conv4
        for b, blk in enumerate(bb.conv1):
            self.layers.append(_SpBlockTrain(blk, 'conv1.%d' % b))
        self.stage_ends.append(len(self.layers) - 1)
        for s, stage in enumerate((bb.conv2, bb.conv3, bb.conv4), start=2):
            down = stage[0]
            self.layers.append(_SpConvBN(down[0], down[1], True, True, 'conv%d.0' % s))
            for b in (1, 2):
                self.layers.append(_SpBlockTrain(stage[b], 'conv%d.%d' % (s, b)))
            self.stage_ends.append(len(self.layers) - 1)
        self.layers.append(_SpConvBN(bb.conv_out[0], bb.conv_out[1], True, True, 'conv_out'))

    def forward(self, features, coords, batch_size, trusted=False):
        """features (N, C) float32, coords (N, 4) int32 [b, z, y, x].  Returns (encoded SparseConvTensor, [x_conv1 .. x_conv4])."""
        if not features.is_cuda:
            raise NotImplementedError('VoxelResBackBone8x: the HIP training path has no CPU form (the voxels are on %s)' % features.device)
        x = spconv.SparseConvTensor(features.float().contiguous(), coords.int().contiguous(), self.m.sparse_shape, batch_size)
        x.trusted_indices = bool(trusted)
        scales = []
        for i, layer in enumerate(self.layers):
            x = layer.forward(x)
            if i in self.stage_ends:
                scales.append(x)
        return x, scales

    def backward(self, dout):
        """dout: (rows of the encoded tensor, 128) float32, overwritten.  The voxel means carry no gradient: returns None."""
        g = dout
        for layer in reversed(self.layers):
            g = layer.backward(g)
        return None
