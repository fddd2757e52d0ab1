"""Device-side graph builders with the call signatures of the torch_cluster / torch_geometric functions the
reference's sparse path uses (models/point_conv.py:5, 341-396; models/continuous_crf_conv.py:53):
knn_graph, knn, radius_graph, fps -- all on top of the exact HIP grid kNN (csrc/knn.hip), one segmented search per graph.

Conventions (PyG): an edge_index is [2, E] with row 0 = source j ("col"), row 1 = target i ("row").
Third-party semantics are unpinned (no version, no tests in the reference): knn_* are exact; radius_graph keeps
the NEAREST `max_num_neighbors` inside the radius (torch_cluster keeps the first it meets); fps starts from the
first point of each cloud unless random_start=True."""
import torch

from ..graph import table_from_index
from ..ops.interp import segment_ptr as _ptr
from ..utils import nearest_neighbors as nn_


def _segments(batch, n):
    """[(start, end)] of each cloud; `batch` must be sorted (PyG convention). None -> one cloud."""
    if batch is None:
        return [(0, n)]
    counts = torch.bincount(batch).tolist()
    out, o = [], 0
    for c in counts:
        if c:
            out.append((o, o + c))
        o += c
    return out


def _knn_table(x, y, k, batch_x, batch_y):
    """int32 [Ny, k] global x rows: for every y row the k nearest x rows of the same cloud, nearest first, -1 where the cloud has fewer
    than k -- ONE search for all clouds (csrc/knn.hip: crfconv_knn_segments_dev)."""
    clouds = 1
    if batch_x is not None or batch_y is not None:
        if batch_x is None or batch_y is None:
            raise ValueError('batch_x and batch_y must be given together')
        clouds = int(torch.maximum(batch_x.max(), batch_y.max())) + 1 if batch_x.numel() and batch_y.numel() else 1
    k = min(k, x.shape[0])              # no cloud has more points than that; the columns left out would be -1
    return nn_.knn_segments_device(x, _ptr(batch_x, x.shape[0], clouds, x.device), y, _ptr(batch_y, y.shape[0], clouds, x.device), k,
                                   out_dtype=torch.int32)


def _knn_segments(x, y, k, batch_x, batch_y):
    """For every y row the k nearest x rows of the same cloud -> (y_index, x_index) global ids, nearest first, cloud by cloud;
    a cloud with fewer than k points gives each of its y rows as many edges as it has points."""
    row, col, _ = _knn_edges(x, y, k, batch_x, batch_y)
    return row, col


def _knn_edges(x, y, k, batch_x, batch_y):
    """_knn_segments and the table the edges were read from."""
    idx = _knn_table(x, y, k, batch_x, batch_y)
    row, slot = (idx >= 0).nonzero(as_tuple=True)           # row-major order
    return row, idx[row, slot].long(), idx


def knn_dilated(x, y, k, dilation, batch_x=None, batch_y=None, generator=None):
    """The reference's random dilation (models/point_conv.py:357-364, 387-394): search k * dilation neighbours, keep k
    of them per query, drawn with replacement by torch.randint.  Drawn per cloud so that a cloud with fewer than
    k * dilation points (the coarse levels of small clouds) draws from the neighbours it has instead of indexing
    past them; the search is one call for all clouds.  -> (y_index, x_index)."""
    seg_x, seg_y = _segments(batch_x, x.shape[0]), _segments(batch_y, y.shape[0])
    idx = _knn_table(x, y, min(k * dilation, max(xe - xs for xs, xe in seg_x)), batch_x, batch_y)
    rows, cols = [], []
    for (xs, xe), (ys, ye) in zip(seg_x, seg_y):
        have = min(k * dilation, xe - xs)
        keep = min(k, have)
        pick = torch.randint(have, (ye - ys, keep), dtype=torch.long, device=x.device, generator=generator)
        rows.append(torch.arange(ys, ye, device=x.device).unsqueeze(1).expand(-1, keep).reshape(-1))
        cols.append(idx[ys:ye].gather(1, pick).reshape(-1).long())
    return torch.cat(rows), torch.cat(cols)


def knn(x, y, k, batch_x=None, batch_y=None):
    """torch_cluster.knn: [2, E] = [y index; x index].  The search's own int32 table ([Ny, k], -1 = no neighbour) rides on the returned
    tensor as `_crf_knn_table` (a padded NeighborTable over the x rows): knn_interpolate blends over it without a second search."""
    row, col, idx = _knn_edges(x, y, k, batch_x, batch_y)
    edges = torch.stack([row, col])
    edges._crf_knn_table = table_from_index(idx, x.shape[0])
    return edges


def knn_graph(pos, k, batch=None, loop=False):
    """torch_cluster.knn_graph (flow source_to_target): [2, E] = [neighbour j; node i]."""
    row, col = _knn_segments(pos, pos, k if loop else k + 1, batch, batch)
    if not loop:
        keep = row != col
        row, col = row[keep], col[keep]
    return torch.stack([col, row])


def radius_graph(pos, r, batch=None, loop=False, max_num_neighbors=32):
    """[2, E] = [neighbour j; node i] for |p_i - p_j| <= r, at most max_num_neighbors per node."""
    k = max_num_neighbors + (0 if loop else 1)
    row, col = _knn_segments(pos, pos, k, batch, batch)
    d2 = ((pos[row] - pos[col]) ** 2).sum(1)
    keep = d2 <= r * r
    if not loop:
        keep &= row != col
    return torch.stack([col[keep], row[keep]])


def fps(pos, batch=None, ratio=0.5, random_start=False):
    """Farthest point sampling per cloud -> sorted global indices (torch_cluster.fps).  One HIP workgroup per cloud
    (csrc/collate.hip: fps_kernel); the number of picks is ceil(ratio * n) per cloud."""
    import math

    from .. import _lib
    from ..graph import ptr, stream_ptr
    segs = _segments(batch, pos.shape[0])
    dev = pos.device
    counts = [e - s for s, e in segs]
    picks = [max(1, int(math.ceil(ratio * n))) if isinstance(ratio, float) else min(int(ratio), n) for n in counts]
    starts = torch.tensor([s for s, _ in segs], dtype=torch.int64, device=dev)
    cnt = torch.tensor(counts, dtype=torch.int64, device=dev)
    npick = torch.tensor(picks, dtype=torch.int64, device=dev)
    ostart = torch.cumsum(npick, 0) - npick
    first = (torch.stack([torch.randint(0, n, (1,)) for n in counts]).reshape(-1).to(dev) if random_start
             else torch.zeros(len(segs), dtype=torch.int64, device=dev))
    p = pos.detach().to(torch.float32).contiguous()
    out = torch.empty(sum(picks), dtype=torch.int64, device=dev)
    ws = torch.empty(pos.shape[0], dtype=torch.float32, device=dev)
    _lib.call('crfconv_fps', ptr(p), len(segs), ptr(starts), ptr(cnt), ptr(ostart), ptr(npick), ptr(first), ptr(ws),
              ptr(out), stream_ptr())
    return out.sort().values            # picks are global rows and clouds are contiguous: one sort orders every cloud's picks
