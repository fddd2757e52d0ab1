"""Device-side graph builders with the call signatures of the torch_cluster / torch_geometric functions the
reference's sparse path uses (models/point_conv.py:5, 341-396; models/continuous_crf_conv.py:53):
knn_graph, knn, radius_graph, fps -- all on top of the exact HIP grid kNN (csrc/knn.hip), one segmented search per graph.

Conventions (PyG): an edge_index is [2, E] with row 0 = source j ("col"), row 1 = target i ("row").
Third-party semantics are unpinned (no version, no tests in the reference): knn_* are exact; radius_graph keeps
the NEAREST `max_num_neighbors` inside the radius (torch_cluster keeps the first it meets); fps starts from the
first point of each cloud unless random_start=True.

Every graph also exists as a finished neighbour table made from the search's own table by one launch (graph.table_from_search): the
`*_table` builders return it without building an edge list, the edge-list builders carry it on the tensor they return
(`_crf_graph_table`, graph.attached_table), and the sparse layers take either.  The random dilation has two builders: knn_dilated
(torch.randint on an edge list, cloud by cloud) and knn_dilated_table (drawn by the finishing launch, keyed by a DilationDraw)."""
import torch

from ..graph import attach_table, table_from_index, table_from_search, table_from_search_dilated
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


class DilationDraw:
    """The key of the device-side dilation draws (knn_dilated_table): a seed, ONE int64 counter word on the device that only the
    kernels read, and a host count of the salts handed out.  Every graph takes the next salt(), so the graphs of a forward draw
    apart; step() advances the device word by a device op -- between forwards, or between the replays of a captured forward, whose
    recorded launches then draw afresh.  Two objects of the same seed that see the same sequence of calls give the same graphs."""

    def __init__(self, seed, device):
        self.seed = int(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self._salts = 0

    def salt(self):
        """The next salt; never repeats within this object."""
        s = self._salts
        self._salts += 1
        return s

    def step(self):
        self.counter.add_(1)
        return self


def knn_dilated_table(x, y, k, dilation, batch_x=None, batch_y=None, *, draw, ptr_x=None, ptr_y=None, self_loops='keep', read_counts=True):
    """The graph of `knn_dilated` as a NeighborTable of the y rows over the x rows, drawn on the device: ONE search of
    min(k * dilation, len(x)) columns and one finishing launch (graph.table_from_search_dilated) that keeps k entries per row, drawn with
    replacement from the row's neighbours -- a row whose cloud has fewer than k points keeps as many picks as the cloud has points.  No
    edge list, no loop over the clouds; with ptr_x / ptr_y (as in `knn_table`) the only host read is the finishing launch's.
    draw: a DilationDraw; the call takes its next salt.  The draws are keyed by the global row, so a batch does not draw what its clouds
    would draw alone, and they are not torch.randint's: `knn_dilated` stays the builder that follows a torch generator.
    self_loops ('keep' / 'drop' / 'last') is applied to the picks, as the reference applies loop=False after its draw.
    read_counts=False: no host read at all -> (full-width table, device counts), for a captured call (graph.table_from_search_dilated)."""
    if k * dilation > 64:
        raise ValueError('k * dilation = %d exceeds the 64 columns of a search' % (k * dilation))
    idx = _knn_table(x, y, k * dilation, batch_x, batch_y, ptr_x, ptr_y)
    if idx.shape[1] == 0:
        idx = torch.full((idx.shape[0], 1), -1, dtype=torch.int32, device=idx.device)
    return table_from_search_dilated(idx, x.shape[0], k, seed=draw.seed, counter=draw.counter, salt=draw.salt(), self_loops=self_loops,
                                     read_counts=read_counts)


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


def pick_counts(n, ratio):
    """Picks per cloud of n points (int64 tensor, any device): a float ratio gives 0 for an empty cloud, else max(1, ceil(ratio * n)) --
    the product formed in float64, so that it is Python's math.ceil(ratio * n) -- and an int ratio min(ratio, n); never more than n."""
    if isinstance(ratio, float):
        want = torch.ceil(n.to(torch.float64) * ratio).to(torch.int64).clamp_(min=1)
    else:
        want = torch.full_like(n, int(ratio))
    return torch.minimum(want, n).clamp_(min=0)


def fps_segments(pos, ptr, ratio, *, first=None, n_out=None, sort=True):
    """Farthest point sampling of S clouds given by their row boundaries `ptr` (device int64 [S + 1], as knn_segments_device takes them)
    -> (idx, ptr_out): global rows of the picks, cloud after cloud, and their boundaries [S + 1] (the exclusive scan of pick_counts).
    first: device int64 [S], each cloud's first pick as a row of the cloud (None: row 0).  sort: each cloud's picks ascending, as `fps`
    returns them; sort=False leaves them in pick order.  ONE launch, one workgroup per cloud (csrc/fps.hip); an empty cloud gets no pick.
    The only host read is the total pick count; with n_out (the caller's promise of that total) there is none and the call can be
    captured and replayed over other positions and other splits with the same total.  Should the promise not hold, picks past n_out
    are dropped, and entries past the real total hold pos.shape[0] (one past the last row)."""
    from .. import _lib
    from ..graph import ptr as dptr, stream_ptr
    dev, N, S = pos.device, pos.shape[0], ptr.numel() - 1
    n = ptr[1:] - ptr[:-1]
    ptr_out = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(pick_counts(n, ratio), 0, out=ptr_out[1:])
    if n_out is None:
        total = int(ptr_out[-1]) if S else 0
        out = torch.empty(total, dtype=torch.int64, device=dev)
    else:
        total = int(n_out)
        ptr_out.clamp_(max=total)                             # no pick is written past the end of `out`, whatever the promise
        out = torch.full((total,), N, dtype=torch.int64, device=dev)
    if S and total:
        npick = ptr_out[1:] - ptr_out[:-1]
        starts, ostart = ptr[:-1].contiguous(), ptr_out[:-1].contiguous()
        first = torch.zeros(S, dtype=torch.int64, device=dev) if first is None else first.to(torch.int64).contiguous()
        p = pos.detach().to(torch.float32).contiguous()
        ws = torch.empty(max(N, 1), dtype=torch.float32, device=dev)      # the running distances of a cloud above 65 536 points
        _lib.call('crfconv_fps', dptr(p), S, dptr(starts), dptr(n.contiguous()), dptr(ostart), dptr(npick.contiguous()), dptr(first),
                  dptr(ws), dptr(out), stream_ptr())
    if not sort or not total:
        return out, ptr_out
    if n_out is None:
        return out.sort().values, ptr_out           # picks are global rows and clouds are contiguous: one sort orders every cloud's picks
    # the same order without torch.sort (not known to replay from a captured graph): count the picks of every row, scan, and entry j is
    # the first row whose running count is above j -- a row picked twice (duplicate points) appears twice, as in the sort
    count = torch.zeros(N + 1, dtype=torch.int64, device=dev).index_add_(0, out, torch.ones_like(out))
    return torch.searchsorted(torch.cumsum(count, 0), torch.arange(total, dtype=torch.int64, device=dev), right=True), ptr_out


def random_first(ptr, generator=None):
    """A uniformly drawn row of every cloud, int64 [S] on ptr's device, in one device op: floor(rand * n), clamped into the cloud
    (0 for an empty one).  generator: a generator of that device."""
    n = ptr[1:] - ptr[:-1]
    u = torch.rand(n.numel(), dtype=torch.float64, device=ptr.device, generator=generator)
    return torch.minimum(torch.floor(u * n).to(torch.int64), n - 1).clamp_(min=0)


def fps(pos, batch=None, ratio=0.5, random_start=False, *, ptr=None, n_out=None, generator=None):
    """Farthest point sampling per cloud -> sorted global indices (torch_cluster.fps).  One HIP workgroup per cloud
    (csrc/fps.hip); the number of picks is ceil(ratio * n) per cloud.  The clouds are given by the sorted `batch` vector (its cloud count
    is one host read), by ptr (device int64 [S + 1] row boundaries) or are one cloud; n_out as in fps_segments.  random_start draws
    every cloud's first row in one device op, floor(rand * n), from `generator` (a device generator) if given."""
    if ptr is None:
        clouds = int(batch.max()) + 1 if batch is not None and batch.numel() else 1
        ptr = _ptr(batch, pos.shape[0], clouds, pos.device)
    elif batch is not None:
        raise ValueError('give the batch vector or the pointer array, not both')
    first = random_first(ptr, generator) if random_start else None
    return fps_segments(pos, ptr, ratio, first=first, n_out=n_out)[0]
