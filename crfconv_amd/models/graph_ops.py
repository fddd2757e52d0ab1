"""Device-side graph builders with the call signatures of the torch_cluster / torch_geometric functions the
reference's sparse path uses (models/point_conv.py:5, 341-396; models/continuous_crf_conv.py:53):
knn_graph, knn, radius_graph, fps -- all on top of the exact HIP grid kNN (csrc/knn.hip), one segmented search per graph.

Conventions (PyG): an edge_index is [2, E] with row 0 = source j ("col"), row 1 = target i ("row").
Third-party semantics are unpinned (no version, no tests in the reference): knn_* are exact; radius_graph keeps
the NEAREST `max_num_neighbors` inside the radius (torch_cluster keeps the first it meets); fps starts from the
first point of each cloud unless random_start=True.

Every graph also exists as a finished neighbour table made from the search's own table by one launch (graph.table_from_search): the
`*_table` builders return it without building an edge list, the edge-list builders carry it on the tensor they return
(`_crf_graph_table`, graph.attached_table), and the sparse layers take either."""
import torch

from ..graph import attach_table, table_from_index, table_from_search
from ..ops._base import state
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


def _knn_table(x, y, k, batch_x, batch_y, ptr_x=None, ptr_y=None):
    """int32 [Ny, k] global x rows: for every y row the k nearest x rows of the same cloud, nearest first, -1 where the cloud has fewer
    than k -- ONE search for all clouds (csrc/knn.hip: crfconv_knn_segments_dev).  ptr_x / ptr_y: device int64 [S + 1] row boundaries
    of the S clouds in place of the batch vectors (no cloud count to read back)."""
    if (ptr_x is None) != (ptr_y is None):
        raise ValueError('ptr_x and ptr_y must be given together')
    if ptr_x is None:
        clouds = 1
        if batch_x is not None or batch_y is not None:
            if batch_x is None or batch_y is None:
                raise ValueError('batch_x and batch_y must be given together')
            clouds = int(torch.maximum(batch_x.max(), batch_y.max())) + 1 if batch_x.numel() and batch_y.numel() else 1
        ptr_x, ptr_y = _ptr(batch_x, x.shape[0], clouds, x.device), _ptr(batch_y, y.shape[0], clouds, x.device)
    elif batch_x is not None or batch_y is not None:
        raise ValueError('give the batch vectors or the pointer arrays, not both')
    k = min(k, x.shape[0])              # no cloud has more points than that; the columns left out would be -1
    return nn_.knn_segments_device(x, ptr_x, y, ptr_y, k, out_dtype=torch.int32)


def _finish(idx, n_src, **how):
    """The search table `idx` as a finished NeighborTable (graph.table_from_search; a search without columns has no edge)."""
    if idx.shape[1] == 0:
        idx = torch.full((idx.shape[0], 1), -1, dtype=torch.int32, device=idx.device)
    return table_from_search(idx, n_src, **how)


def _radius_cut(pos, r):
    pos = pos.detach().to(torch.float32).contiguous()
    return dict(pos_src=pos, pos_tgt=pos, radius=r)


def knn_table(x, y, k, batch_x=None, batch_y=None, *, ptr_x=None, ptr_y=None):
    """The graph of `knn` as a NeighborTable of the y rows over the x rows: one search, one finishing launch, no edge list.  Equals
    graph.table_from_edges(e[0], e[1], len(y), len(x)) of e = knn(x, y, k, batch_x, batch_y)."""
    return _finish(_knn_table(x, y, k, batch_x, batch_y, ptr_x, ptr_y), x.shape[0])


def radius_table(x, y, r, k, batch_x=None, batch_y=None, *, ptr_x=None, ptr_y=None):
    """knn_table cut at the radius r: for every y row its nearest x rows of the same cloud inside r, at most k."""
    idx = _knn_table(x, y, k, batch_x, batch_y, ptr_x, ptr_y)
    return _finish(idx, x.shape[0], pos_src=x.detach().to(torch.float32).contiguous(), pos_tgt=y.detach().to(torch.float32).contiguous(),
                   radius=r)


def knn_graph_table(pos, k, batch=None, loop=False, *, ptr=None):
    """The graph of `knn_graph` as a NeighborTable (targets = row 1 of its edge list): one search, one finishing launch."""
    idx = _knn_table(pos, pos, k if loop else k + 1, batch, batch, ptr, ptr)
    return _finish(idx, pos.shape[0], self_loops='keep' if loop else 'drop')


def radius_graph_table(pos, r, batch=None, loop=False, max_num_neighbors=32, *, ptr=None):
    """The graph of `radius_graph` as a NeighborTable (targets = row 1 of its edge list): one search, one finishing launch whose
    radius cut forms the squared distance like the search does."""
    idx = _knn_table(pos, pos, max_num_neighbors + (0 if loop else 1), batch, batch, ptr, ptr)
    return _finish(idx, pos.shape[0], self_loops='keep' if loop else 'drop', **_radius_cut(pos, r))


def _carry(edges, target_row, idx, n_src, **how):
    """`edges` with the finished table of its graph attached -- unless ops.state.no_graph_tables, or the table's edge count is not the
    list's (a distance within rounding of the radius that the framework's expression and the kernel's cut place on different sides)."""
    if state.no_graph_tables:
        return edges
    table = _finish(idx, n_src, **how)
    return attach_table(edges, table, target_row) if table.n_edges == edges.shape[1] else edges


def _knn_edges(x, y, k, batch_x, batch_y):
    """For every y row the k nearest x rows of the same cloud -> (y_index, x_index) global ids, nearest first, cloud by cloud (a cloud
    with fewer than k points gives each of its y rows as many edges as it has points), and the table the edges were read from."""
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
    tensor as `_crf_knn_table` (a padded NeighborTable over the x rows): knn_interpolate blends over it without a second search.  The
    finished table (knn_table) rides on it as well."""
    row, col, idx = _knn_edges(x, y, k, batch_x, batch_y)
    edges = torch.stack([row, col])
    edges._crf_knn_table = table_from_index(idx, x.shape[0])
    return _carry(edges, 0, idx, x.shape[0])


def knn_graph(pos, k, batch=None, loop=False):
    """torch_cluster.knn_graph (flow source_to_target): [2, E] = [neighbour j; node i]."""
    row, col, idx = _knn_edges(pos, pos, k if loop else k + 1, batch, batch)
    if not loop:
        keep = row != col
        row, col = row[keep], col[keep]
    return _carry(torch.stack([col, row]), 1, idx, pos.shape[0], self_loops='keep' if loop else 'drop')


def radius_graph(pos, r, batch=None, loop=False, max_num_neighbors=32):
    """[2, E] = [neighbour j; node i] for |p_i - p_j| <= r, at most max_num_neighbors per node."""
    k = max_num_neighbors + (0 if loop else 1)
    row, col, idx = _knn_edges(pos, pos, k, batch, batch)
    d2 = ((pos[row] - pos[col]) ** 2).sum(1)
    keep = d2 <= r * r
    if not loop:
        keep &= row != col
    return _carry(torch.stack([col[keep], row[keep]]), 1, idx, pos.shape[0], self_loops='keep' if loop else 'drop', **_radius_cut(pos, r))


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
