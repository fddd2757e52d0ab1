"""Voxel-grid subsampling of ragged batches on the device, with the inverse map (csrc/grid_subsample.hip).

The reference subsamples every raw cloud on a grid before anything else (``_grid_sub_sampling``: datasets/s3dis_dataset.py:296,
semantic3d_dataset.py:332/340/362, through the CPython extension ``cpp_subsampling``): a voxel of edge ``size`` becomes one point, the
barycentre of its points, with the mean of their features and the most frequent of their labels.  ``grid_subsample`` does that for all
clouds of a batch in one call -- each cloud on the grid of its own bounding box, as if it had been subsampled alone, bit for bit the rows
``utils.cpp_subsampling.compute`` returns for it -- and keeps what the sort knows anyway, the voxel of every input point:

    sample = grid.grid_subsample(pos, ptr, size=0.04, x=colours, y=labels)
    split = blocks.sliding_blocks(sample.pos, sample.ptr, **blocks.S3DIS)       # ... the network over the blocks, BlockVotes ...
    pred_raw = votes.result()[1][sample.inverse]                                # the sub-cloud's predictions on the RAW points

There is one host read (the number of voxels and the status, which size the results) and no Python loop over clouds.
"""
import collections

import torch

from . import _lib

_LIMIT = 1 << 31
_STATUS_BAD_PTR, _STATUS_OVERFLOW = 1, 4

GridSample = collections.namedtuple('GridSample', 'pos ptr x y inverse counts')
GridSample.__doc__ = """The voxels of ``grid_subsample``, device tensors: pos [M, 3] float32 barycentres; ptr [S + 1] int64, cloud s = rows
ptr[s] .. ptr[s + 1] (an empty cloud repeats an entry); x [M, F] float32 feature means or None; y label modes (the smallest label on a
tie) with the caller's dtype and number of dimensions, or None; inverse [N] int64, the row of every input point's voxel; counts [M] int32,
the points per voxel.  Rows come cloud by cloud, in ascending voxel key iX + NX iY + NX NY iZ inside a cloud."""


def _host_ptr(ptr, N):
    """ptr given on the host (a list or a host tensor), checked here: int64 tensor [S + 1]."""
    t = ptr if torch.is_tensor(ptr) else torch.tensor(list(ptr), dtype=torch.int64)
    if not (t.dtype == torch.int64 and t.dim() == 1 and t.numel() >= 1):
        raise ValueError('grid_subsample: ptr must be int64 [S + 1]')
    v = t.tolist()
    if v[0] != 0 or v[-1] != N or any(b < a for a, b in zip(v, v[1:])):
        raise ValueError('grid_subsample: ptr must start at 0, end at N = %d and be non-decreasing' % N)
    return t


def grid_subsample(pos, ptr=None, *, size, x=None, y=None):
    """The voxels of edge ``size`` of the clouds of pos [N, 3] (float32, device) given by ptr [S + 1] (int64: a device tensor, a host
    tensor or a list; None: one cloud) -> GridSample.  x [N, F] float32 and y [N] or [N, L] int32 / int64 (values inside int32) are
    optional per-point features and labels.

    Per cloud, in the reference's float32 operations (grid_subsampling.cpp:27-31, :53-56, :84-104): origin = floor(min / size) * size,
    voxel of a point = floor((p - origin) / size) per axis, its key iX + NX iY + NX NY iZ; a voxel's barycentre and feature mean are sums
    in ascending row order, the label the mode of its column.  The results have room for N rows and are returned cut to the M voxels.

    Limits: positions finite; N below 2^31; with more than one cloud the clouds' grid cell counts NX NY NZ must fit one 64-bit key
    together (ValueError otherwise; one cloud alone wraps around as the reference's size_t does)."""
    from .graph import ptr as p_, require_gpu, stream_ptr, to_device
    if not (torch.is_tensor(pos) and pos.dim() == 2 and pos.shape[1] == 3 and pos.dtype == torch.float32):
        raise ValueError('grid_subsample: pos must be a float32 tensor [N, 3]')
    N = pos.shape[0]
    if N >= _LIMIT:
        raise ValueError('grid_subsample: N = %d is not below 2^31' % N)
    size = float(size)
    if not (size > 0.0 and size != float('inf') and float(torch.tensor(size, dtype=torch.float32)) > 0.0):
        raise ValueError('grid_subsample: size must be positive (and finite, also as float32), got %r' % (size,))
    if x is not None and not (torch.is_tensor(x) and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] == N):
        raise ValueError('grid_subsample: x must be a float32 tensor [N, F] with N = %d rows' % N)
    if y is not None and not (torch.is_tensor(y) and y.dim() in (1, 2) and y.dtype in (torch.int32, torch.int64) and y.shape[0] == N):
        raise ValueError('grid_subsample: y must be an int32 or int64 tensor [N] or [N, L] with N = %d rows' % N)
    if ptr is None:
        ptr = torch.tensor([0, N], dtype=torch.int64)
    elif not (torch.is_tensor(ptr) and ptr.is_cuda):
        ptr = _host_ptr(ptr, N)
    elif not (ptr.dtype == torch.int64 and ptr.dim() == 1 and ptr.numel() >= 1):
        raise ValueError('grid_subsample: ptr must be int64 [S + 1]')
    S = ptr.numel() - 1
    if S == 0 and N:
        raise ValueError('grid_subsample: ptr names no cloud but pos has %d rows' % N)
    if not pos.is_cuda:
        raise ValueError('grid_subsample: pos must be on the device (got %s); there is no CPU path' % pos.device)
    dev = pos.device
    for name, t in (('x', x), ('y', y), ('ptr', ptr if ptr.is_cuda else None)):
        if t is not None and t.device != dev:
            raise ValueError('grid_subsample: %s is on %s, pos on %s' % (name, t.device, dev))
    ptr = to_device(ptr, dev).contiguous()
    require_gpu(ptr)
    F = x.shape[1] if x is not None else 0
    L = (1 if y.dim() == 1 else y.shape[1]) if y is not None else 0
    i64 = torch.int64
    if N == 0:                                             # every cloud empty: nothing to launch
        e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)          # noqa: E731
        return GridSample(e(0, 3), to_device(torch.zeros(S + 1, dtype=i64), dev), None if x is None else e(0, F),
                          None if y is None else e(*((0,) + tuple(y.shape[1:])), dtype=y.dtype), e(0, dtype=i64), e(0, dtype=torch.int32))
    pos = pos.detach().contiguous()
    feats = x.detach().contiguous() if F else None
    labels = y.reshape(N, L).to(torch.int32).contiguous() if L else None
    out_pos = torch.empty((N, 3), dtype=torch.float32, device=dev)
    out_x = torch.empty((N, F), dtype=torch.float32, device=dev) if F else None
    out_y = torch.empty((N, L), dtype=torch.int32, device=dev) if L else None
    out_ptr = torch.empty(S + 1, dtype=i64, device=dev)
    inverse = torch.empty(N, dtype=i64, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=i64, device=dev)
    nbytes = _lib.call('crfconv_grid_subsample_segments_workspace', N, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call('crfconv_grid_subsample_segments', p_(pos), N, p_(ptr), S, p_(feats), F, p_(labels), L, size, N, p_(ws), nbytes, p_(out_pos),
              p_(out_x), p_(out_y), p_(out_ptr), p_(inverse), p_(counts), p_(totals), stream_ptr())
    M, status = totals.tolist()                                                            # THE host read
    if status & _STATUS_BAD_PTR:
        raise ValueError('grid_subsample: ptr must start at 0, end at N = %d and be non-decreasing' % N)
    if status & _STATUS_OVERFLOW:
        raise ValueError('grid_subsample: the grid cell counts of the clouds do not fit one 64-bit key together (size = %g is too small '
                         'for their extent)' % size)
    if x is not None:
        out_x = out_x[:M] if F else torch.empty((M, 0), dtype=torch.float32, device=dev)
    if y is not None:
        out_y = (out_y[:M] if L else torch.empty((M, 0), dtype=torch.int32, device=dev)).to(y.dtype)
        out_y = out_y.reshape(M) if y.dim() == 1 else out_y
    return GridSample(out_pos[:M], out_ptr, out_x, out_y, inverse, counts[:M])
