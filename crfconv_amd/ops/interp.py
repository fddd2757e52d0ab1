"""kNN interpolation (torch_geometric.nn.knn_interpolate): the inverse-squared-distance blend and its transpose (csrc/interp.hip)."""
import torch

from .. import _lib
from ..graph import ptr, require_gpu, stream_ptr, table_from_index
from ._base import _f32c


def _check(x, pos_x, pos_y, table):
    require_gpu(x, pos_x, pos_y, table.idx32)
    for t in (x, pos_x, pos_y):
        if t.dtype != torch.float32:
            raise _lib.CrfConvError('interpolate: float32 tensors only (got %s)' % t.dtype)
    if (x.dim() != 2 or x.shape[1] < 1 or pos_x.shape != (x.shape[0], 3) or pos_y.shape != (table.m_tgt, 3)
            or table.m_src != x.shape[0]):
        raise _lib.CrfConvError('interpolate: x [n_x, C], pos_x [n_x, 3], pos_y [n_y, 3] and a table of n_y rows over n_x sources '
                                '(got %s, %s, %s, table %d x %d over %d)' % (tuple(x.shape), tuple(pos_x.shape), tuple(pos_y.shape),
                                                                            table.m_tgt, table.K, table.m_src))


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos_x, pos_y, table, need_grad):
        x, pos_x, pos_y = _f32c(x), _f32c(pos_x), _f32c(pos_y)
        n_y, n_x, C = table.m_tgt, x.shape[0], x.shape[1]
        out = torch.empty((n_y, C), dtype=torch.float32, device=x.device)
        coef = torch.empty((n_y, table.K), dtype=torch.float32, device=x.device) if need_grad else None
        _lib.call('crfconv_interpolate', ptr(x), ptr(pos_x), ptr(pos_y), ptr(table.idx32), table.K, n_y, n_x, C, ptr(coef), None, None,
                  ptr(out), stream_ptr())
        ctx.table, ctx.n_x = table, n_x
        ctx.save_for_backward(coef)
        return out

    @staticmethod
    def backward(ctx, gout):
        (coef,) = ctx.saved_tensors
        table = ctx.table
        g = _f32c(gout)
        rev_ptr, rev_eid = table.reverse
        dx = torch.empty((ctx.n_x, g.shape[1]), dtype=torch.float32, device=g.device)
        _lib.call('crfconv_interpolate', ptr(g), None, None, None, table.K, table.m_tgt, ctx.n_x, g.shape[1], ptr(coef), ptr(rev_ptr),
                  ptr(rev_eid), ptr(dx), stream_ptr())
        return dx, None, None, None, None


def interpolate(x, pos_x, pos_y, table):
    """out[i] = sum_s w_is x[table[i, s]] / sum_s w_is,  w_is = 1 / max(|pos_y[i] - pos_x[table[i, s]]|^2, 1e-16), over the row's valid
    slots in slot order: x [n_x, C], pos_x [n_x, 3], pos_y [n_y, 3] float32 CUDA tensors, `table` a NeighborTable of n_y rows (entries
    outside [0, n_x) = no neighbour) -> [n_y, C].  One launch forward (the normalised weights are kept only when x needs a gradient), one
    launch backward over table.reverse: no atomics, the same bits in every run.  The gradient goes to x only -- the positions get none, as
    in torch_geometric, which forms the weights under no_grad.  A row without any neighbour is zero (the framework composition gave NaN)."""
    _check(x, pos_x, pos_y, table)
    if table.m_tgt == 0 or x.shape[0] == 0:
        return x.new_zeros((table.m_tgt, x.shape[1]))          # nothing to launch: no row, or no source for any row
    return _Interpolate.apply(x, pos_x.detach(), pos_y.detach(), table, x.requires_grad and torch.is_grad_enabled())


def segment_ptr(batch, n, clouds, device):
    """int64 [clouds + 1] row boundaries of a sorted `batch` vector over n rows (None -> one cloud), made on the device."""
    if batch is None:
        return torch.tensor([0, n], dtype=torch.int64, device=device)
    out = torch.zeros(clouds + 1, dtype=torch.int64, device=device)
    out[1:] = torch.cumsum(torch.bincount(batch, minlength=clouds), 0)
    return out


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, *, ptr_x=None, ptr_y=None):
    """torch_geometric.nn.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k): ONE segmented exact search (int32 table, -1 where a
    cloud has fewer than k sources), then `interpolate` over it.  With ptr_x / ptr_y (device int64 [S + 1] row boundaries of the S clouds)
    in place of the batch vectors nothing is read back: the forward can be captured and replayed over other contents of the same shapes.
    The batch vectors must be sorted; their cloud count is one host read."""
    from ..utils import nearest_neighbors as nn_
    require_gpu(x, pos_x, pos_y)
    if (ptr_x is None) != (ptr_y is None):
        raise ValueError('ptr_x and ptr_y must be given together')
    if ptr_x is None:
        if (batch_x is None) != (batch_y is None):
            raise ValueError('batch_x and batch_y must be given together')
        clouds = 1
        if batch_x is not None and batch_x.numel() and batch_y.numel():
            clouds = int(torch.maximum(batch_x.max(), batch_y.max())) + 1
        ptr_x = segment_ptr(batch_x, pos_x.shape[0], clouds, pos_x.device)
        ptr_y = segment_ptr(batch_y, pos_y.shape[0], clouds, pos_x.device)
    elif batch_x is not None or batch_y is not None:
        raise ValueError('give the batch vectors or the pointer arrays, not both')
    k = max(1, min(int(k), pos_x.shape[0]))            # no cloud has more sources than that; the columns left out would be -1
    idx = nn_.knn_segments_device(pos_x, ptr_x, pos_y, ptr_y, k, out_dtype=torch.int32)
    return interpolate(x, pos_x, pos_y, table_from_index(idx, pos_x.shape[0]))
