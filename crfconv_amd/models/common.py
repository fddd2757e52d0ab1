"""Building blocks with the reference's names, signatures and state_dict layout
(models/common.py:9-40, 89-97).  FastBatchNorm1d mirrors the torch_points3d module the
reference imports (BatchNorm1d kept as ``.batch_norm``, statistics over every leading dim)."""
import torch
import torch.nn as nn

from .. import ops
from ..graph import require_gpu
from . import graph_ops


def _fps_graph(pos, batch, k, r, ptr):
    """(idx, table, clouds): the farthest point picks of every cloud, the NeighborTable of the picks over all points (their k nearest
    of the same cloud; -1 where a cloud has fewer) and the picks' cloud description -- batch[idx], None for one cloud, or with `ptr`
    (device int64 [S + 1] in place of `batch`) the picks' own ptr, without a cloud count read back."""
    require_gpu(pos)
    if ptr is not None:
        if batch is not None:
            raise ValueError('give the batch vector or the pointer array, not both')
        idx, ptr_out = graph_ops.fps_segments(pos, ptr, r)
        return idx, graph_ops.knn_table(pos, pos[idx], k, ptr_x=ptr, ptr_y=ptr_out), ptr_out
    idx = graph_ops.fps(pos, batch, ratio=r)
    sub = None if batch is None else batch[idx]
    return idx, graph_ops.knn_table(pos, pos[idx], k, batch, sub), sub


def fps_pooling(pos, x, edge_attr, batch=None, k=16, r=0.5, reduce='sum', *, ptr=None):
    """models/common.py:9-15: farthest point sampling at ratio r, then every pick pools the features of its k nearest points with
    `reduce` -> (x, pos, edge_attr, batch) of the picks.  The graph is a NeighborTable and the reduction ops.neighbor_pool: no edge
    list.  batch=None is one cloud (the returned batch is None); with `ptr` the last item is the picks' ptr."""
    if reduce not in ('max', 'mean', 'add', 'sum'):
        raise ValueError("fps_pooling: reduce must be one of 'max', 'mean', 'add', 'sum' (got %r)" % (reduce,))
    idx, table, sub = _fps_graph(pos, batch, k, r, ptr)
    return ops.neighbor_pool(x, table, reduce), pos[idx], edge_attr[idx], sub


def fps_max_pooling(pos, x, batch=None, k=16, r=0.5, *, ptr=None):
    """models/common.py:18-23: fps_pooling with the max, without edge attributes -> (x, pos, batch)."""
    idx, table, sub = _fps_graph(pos, batch, k, r, ptr)
    return ops.neighbor_pool(x, table, 'max'), pos[idx], sub


class FastBatchNorm1d(nn.Module):
    def __init__(self, num_features, momentum=0.1, **kwargs):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(num_features, momentum=momentum, **kwargs)

    def forward(self, x):
        if x.dim() not in (2, 3):
            raise ValueError('Non supported number of dimensions {}'.format(x.dim()))
        bn = self.batch_norm
        if not bn.affine or x.dtype != torch.float32:
            raise ops._lib.CrfConvError('FastBatchNorm1d: affine float32 BatchNorm only (the kernels of csrc/bn.hip); got affine=%s, %s'
                                        % (bn.affine, x.dtype))
        return ops.bn_act(x, bn, self.training)          # statistics over every leading dim, one stats + one apply pass (csrc/bn.hip)


class MLP(nn.Module):
    """Linear(bias = not bn) -> BatchNorm -> activation (models/common.py:26-40)."""

    def __init__(self, in_channels, out_channels, bn=True, activation=None):
        super(MLP, self).__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=not bn)
        self.bn = FastBatchNorm1d(out_channels) if bn else None
        self.activation = activation

    def forward(self, x, *args, **kwargs):
        require_gpu(x)                                    # every layer of the path runs on the device; no CPU path
        co = self.lin.out_features
        fusable = (self.bn is not None and x.dtype == torch.float32 and co % 4 == 0 and co <= 1024
                   and self.bn.batch_norm.affine
                   and (self.activation is None or isinstance(self.activation, nn.LeakyReLU)))
        if fusable:      # Linear (MFMA, BatchNorm statistics in its epilogue) -> BatchNorm + LeakyReLU in one pass
            slope = 1.0 if self.activation is None else self.activation.negative_slope
            if ops.mlp_block_ok(x, self.lin.weight, self.lin.bias, self.bn.batch_norm, self.training):
                return ops.mlp_block(x, self.lin.weight, self.bn.batch_norm, slope)      # one autograd node, fused backward
            records = None
            if self.training:
                x, records = ops.linear(x, self.lin.weight, self.lin.bias, want_stats=True)
            else:
                x = ops.linear(x, self.lin.weight, self.lin.bias)
            slope = 1.0 if self.activation is None else self.activation.negative_slope
            return ops.bn_act(x, self.bn.batch_norm, self.training, slope, records=records)
        x = ops.linear(x, self.lin.weight, self.lin.bias)
        if self.bn is not None:
            x = self.bn(x)                                # FastBatchNorm1d: ops.bn_act (raises for what csrc/bn.hip does not take)
        if self.activation is not None:
            x = self.activation(x)                        # an activation module other than LeakyReLU is the caller's own
        return x


def mlp_fork(mlp, x, input_mask=None):
    """(mlp(x), x') for an input with a second consumer (the ResNet block: lin_in(x) and shortcut(x),
    models/point_conv_big.py:83-88).  x' is x; where the fused block applies it is an alias whose gradient is added inside the
    block's backward while dX is written, instead of by an accumulation pass of autograd's (ops._MLPBlock, fork).
    input_mask: the ops.JoinMask of the join that produced x, from a caller who knows that x has no use outside this fork chain."""
    if (mlp.training and mlp.bn is not None and x.dtype == torch.float32 and mlp.bn.batch_norm.affine and x.requires_grad
            and mlp.lin.out_features % 4 == 0 and mlp.lin.out_features <= 1024
            and (mlp.activation is None or isinstance(mlp.activation, nn.LeakyReLU))
            and ops.mlp_block_ok(x, mlp.lin.weight, mlp.lin.bias, mlp.bn.batch_norm, True)):
        require_gpu(x)
        slope = 1.0 if mlp.activation is None else mlp.activation.negative_slope
        return ops.mlp_block(x, mlp.lin.weight, mlp.bn.batch_norm, slope, fork=True, input_mask=input_mask)
    return mlp(x), x


def _group_spec(mlp, x):
    """(W, BatchNorm1d, slope) of an MLP that the fused training-mode blocks take -- Linear without bias, affine BatchNorm, no or a
    LeakyReLU activation --, else None."""
    if not (isinstance(mlp, MLP) and mlp.training and mlp.bn is not None and mlp.lin.bias is None and x.dtype == torch.float32
            and mlp.bn.batch_norm.affine and (mlp.activation is None or isinstance(mlp.activation, nn.LeakyReLU))):
        return None
    return mlp.lin.weight, mlp.bn.batch_norm, (1.0 if mlp.activation is None else mlp.activation.negative_slope)


def mlp_group(pairs, shared=False, input_mask=None):
    """[(mlp, x, fork)] -> [mlp(x) or (mlp(x), x_alias)] with all the MLPs in ONE autograd node of two launches each way
    (ops.mlp_group: coarse-level training blocks whose inputs are all ready), or None when that form does not apply to every member
    -- the caller then runs them one by one.  input_mask (shared): as mlp_fork's, for the tensor the first two MLPs read."""
    blocks = []
    for mlp, x, fork in pairs:
        spec = _group_spec(mlp, x)
        if spec is None:
            return None
        require_gpu(x)
        blocks.append((x, spec[0], spec[1], spec[2], fork))
    return ops.mlp_group(blocks, shared=shared, input_mask=input_mask)


def mlp_join(mlp, x, skip, slope=0.01, mask=None, combine=None):
    """leaky_relu(mlp(x) + skip, slope) for an MLP without activation -- the tail of a ResNet block
    (models/point_conv_big.py:84-88).  One fused node (BatchNorm + add + LeakyReLU in a single pass) where it applies
    (training, MFMA-sized rows), else the module followed by ops.add_lrelu.  mask: the ops.JoinMask the fused node shares with the
    node that writes its output's gradient (left unarmed by the fallback).  combine: the ops.CombineHandle of the PointConv layer whose
    (possibly unfilled) output x is -- taken by the fused node, else the combine is launched before anything reads x."""
    if (mlp.training and mlp.bn is not None and mlp.activation is None and mlp.lin.bias is None and x.dtype == torch.float32
            and mlp.bn.batch_norm.affine and mlp.lin.out_features % 4 == 0):
        out = ops.mlp_block_join(x, mlp.lin.weight, mlp.bn.batch_norm, skip, slope, mask=mask, combine=combine)
        if out is not None:
            return out
    if combine is not None:
        combine.flush()
    return ops.add_lrelu(mlp(x), skip, slope)


class Base(nn.Module):
    """state_dict round trip (models/common.py:89-97)."""

    def save(self, filename):
        torch.save(self.state_dict(), filename)

    # A self-capturing model (train.autograph_forward, train.autograph_eval_forward) keeps its private graph runners -- one for training
    # mode, one for eval mode under no_grad -- in its instance dictionary, outside the module tree.  Their graphs hold device addresses: a
    # copy of the model starts without them, and whatever moves or casts the parameters (to(), float(), cuda()) drops them -- the next
    # call captures again.
    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop('_autograph', None)
        state.pop('_autograph_eval', None)
        return state

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop('_autograph', None)
        self.__dict__.pop('_autograph_eval', None)
        return super()._apply(fn, *args, **kwargs)

    def load(self, filename):
        self.load_state_dict(torch.load(filename))
