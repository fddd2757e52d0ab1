"""-m gpu: neighbour tables straight from the search (csrc/graph_table.hip, graph.table_from_search, the *_table builders of
models/graph_ops.py) against the edge-list composition they replace, run in the same test: the table of every graph must be the one
graph.table_from_edges groups out of the corresponding edge list -- torch.equal, no tolerance: it is the same table, and it feeds
the same kernels."""
import copy

import numpy as np
import pytest
import torch

import _seeded as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_table(a, b):
    """The fields a consumer reads."""
    assert a.K == b.K and tuple(a.idx32.shape) == tuple(b.idx32.shape), (tuple(a.idx32.shape), tuple(b.idx32.shape))
    assert a.idx32.dtype == torch.int32 and a.idx32.is_contiguous()
    assert torch.equal(a.idx32, b.idx32)
    assert a.n_edges == b.n_edges, (a.n_edges, b.n_edges)
    assert (a.B, a.n_tgt, a.n_src, a.padded) == (b.B, b.n_tgt, b.n_src, b.padded) and a.padded and a.B == 1


def tie_free(pos64, r, pairs):
    """In float64 no candidate pair (i, j) lies within 1e-6 r^2 of the radius: the kernel's singly rounded sum and the
    framework's expression cannot fall on different sides of it."""
    r2 = float(r) * float(r)
    d2 = ((pos64[pairs[0]] - pos64[pairs[1]]) ** 2).sum(1)
    return bool((np.abs(d2 - r2) > 1e-6 * r2).all())


# ------------------------------------------------------------------------------------------ the kernel against the composition
def synthetic(n, K, seed):
    """[n, K] random rows of n sources with holes: row i draws from i - 10 .. i + 10 (mod n; so some entries come twice); a quarter
    of the entries are -1 or past the range, wherever they fall; every seventh row is empty; every third row holds its own index."""
    tab = ((np.arange(n)[:, None] + S.integers(seed, 'tab', (n, K), -10, 11)) % n).astype(np.int32)
    hole = S.uniform(seed, 'hole', (n, K), 0, 1)
    tab[hole < 0.2] = -1
    tab[(hole >= 0.2) & (hole < 0.25)] = n + 3
    col = S.integers(seed, 'selfcol', (n,), 0, K)
    own = np.arange(n) % 3 == 0
    tab[own, col[own]] = np.arange(n, dtype=np.int32)[own]
    tab[np.arange(n) % 7 == 3] = -1
    return tab


def kernel_cloud(n, seed):
    """Points of the unit box, every fiftieth moved far away to a place of its own: with r = 2 (above the box's diagonal) a pair of
    two points is cut exactly when one of them is such a point -- its row loses every entry, rows that draw it lose some, the others
    none."""
    pos = S.make_cloud(seed, n).astype(np.float32)
    far = np.arange(n) % 50 == 7
    pos[far, 0] += (np.float32(10.0) * (1 + np.arange(n, dtype=np.float32)))[far]
    return pos


def composition(tab, n_src, mode, pos, r):
    """The path the kernel replaces: the table masked into an edge list, the framework's radius expression and self filter,
    arange loops appended for mode 2 (DepthwiseSeparablePointConv.forward), then table_from_edges."""
    from crfconv_amd.graph import table_from_edges
    n = tab.shape[0]
    row, slot = ((tab >= 0) & (tab < n_src)).nonzero(as_tuple=True)
    col = tab[row, slot].long()
    keep = torch.ones_like(row, dtype=torch.bool)
    if r is not None:
        keep &= ((pos[row] - pos[col]) ** 2).sum(1) <= r * r
    if mode:
        keep &= row != col
    row, col = row[keep], col[keep]
    if mode == 2:
        loops = torch.arange(n, dtype=torch.long, device=tab.device)
        row, col = torch.cat([row, loops]), torch.cat([col, loops])
    return table_from_edges(row, col, n, n_src)


@pytest.mark.parametrize('K', [1, 3, 16, 17, 33, 64])
def test_kernel_equals_the_composition(K):
    """Both sides of every lane-group width (1, 4, 16, 32, 64, 64), one row, a last partial workgroup (257 = 256 + 1 rows at one row
    per lane, 1005 at every width), all self modes, with and without the radius cut."""
    from crfconv_amd.graph import table_from_search
    R = 2.0
    for n in (1, 257, 1005):
        tab_np, pos_np = synthetic(n, K, 100 * K + n), kernel_cloud(n, 7 * K + n)
        row, slot = ((tab_np >= 0) & (tab_np < n)).nonzero()
        assert tie_free(pos_np.astype(np.float64), R, (row, tab_np[row, slot]))
        tab, pos = t(tab_np), t(pos_np)
        for mode, name in enumerate(('keep', 'drop', 'last')):
            for r in (None, R):
                if K == 64 and mode == 2:
                    continue                                     # degree 65: test_degree_above_the_maximum_raises
                want = composition(tab, n, mode, pos, r)
                got = table_from_search(tab, n, pos_src=pos, pos_tgt=pos, radius=r, self_loops=name)
                same_table(got, want)
                if n == 1005 and r is not None and mode == 1:
                    deg, full = (want.idx32 >= 0).sum(1), ((tab >= 0) & (tab < n) & (tab != torch.arange(n, device=DEV)[:, None])).sum(1)
                    assert int(((deg == 0) & (full > 0)).sum()) > 0 and int(((deg == full) & (full > 0)).sum()) > 0
                    assert 0 < want.n_edges < int(full.sum())
    # mode 0 over another number of sources (a bipartite table), entries past n_src are holes
    tab_np = synthetic(257, K, 900 + K)
    tab = t(tab_np)
    same_table(table_from_search(tab, 200), composition(tab, 200, 0, None, None))
    with pytest.raises(ValueError):
        table_from_search(tab, 200, self_loops='drop')


@pytest.mark.parametrize('K,n,mode', [(64, 8195, 1), (16, 33000, 2), (1, 262444, 0), (3, 65536 + 64 * 1024, 2)])
def test_kernel_walks_on_over_the_tiles(K, n, mode):
    """More row tiles than the launch has workgroups (1024): a workgroup makes several trips, the last one partial or missing -- 2049
    tiles of 4 rows, 2063 of 16, 1026 of 256, and exactly two trips for every workgroup (2048 tiles of 64 rows)."""
    from crfconv_amd.graph import table_from_search
    R = 2.0
    tab_np, pos_np = synthetic(n, K, 300 + K), kernel_cloud(n, 300 + K)
    row, slot = ((tab_np >= 0) & (tab_np < n)).nonzero()
    assert tie_free(pos_np.astype(np.float64), R, (row, tab_np[row, slot]))
    tab, pos = t(tab_np), t(pos_np)
    for r in (None, R):
        same_table(table_from_search(tab, n, pos_src=pos, pos_tgt=pos, radius=r, self_loops=('keep', 'drop', 'last')[mode]),
                   composition(tab, n, mode, pos, r))


def test_degree_above_the_maximum_raises():
    """K = 64, self appended to a row that does not hold its own index: degree 65, the error table_from_edges raises."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import table_from_search
    n = 70
    tab = t(((np.arange(n)[:, None] + 1 + np.arange(64)[None, :]) % n).astype(np.int32))          # row i: i + 1 .. i + 64 (mod 70), never i
    with pytest.raises(_lib.CrfConvError, match='in-degree 65 exceeds the supported maximum 64') as got:
        table_from_search(tab, n, self_loops='last')
    with pytest.raises(_lib.CrfConvError) as want:
        composition(tab, n, 2, None, None)
    assert str(got.value) == str(want.value)
    same_table(table_from_search(tab, n, self_loops='drop'), composition(tab, n, 1, None, None))       # 64 is fine
    own = tab.clone()
    own[:, 5] = torch.arange(n, dtype=torch.int32, device=DEV)                                     # every row holds itself: 63 + 1
    same_table(table_from_search(own, n, self_loops='last'), composition(own, n, 2, None, None))


def test_no_edge_at_all_and_the_reverse_csr():
    from crfconv_amd.graph import table_from_search
    n, K = 257, 16
    tab_np, pos_np = synthetic(n, K, 41), S.make_cloud(41, n)
    tab_np[tab_np == np.arange(n)[:, None]] = -1                 # no row holds itself: every candidate pair is two distinct points
    row, slot = ((tab_np >= 0) & (tab_np < n)).nonzero()
    d2 = ((pos_np[row].astype(np.float64) - pos_np[tab_np[row, slot]].astype(np.float64)) ** 2).sum(1)
    r = 0.5 * float(np.sqrt(d2.min()))                           # below every candidate distance
    assert r > 0 and tie_free(pos_np.astype(np.float64), r, (row, tab_np[row, slot]))
    assert tie_free(pos_np.astype(np.float64), 0.6, (row, tab_np[row, slot]))
    tab, pos = t(tab_np), t(pos_np)
    for name, mode in (('keep', 0), ('drop', 1)):
        got = table_from_search(tab, n, pos_src=pos, pos_tgt=pos, radius=r, self_loops=name)
        assert tuple(got.idx32.shape) == (n, 1) and int((got.idx32 != -1).sum()) == 0 and got.n_edges == 0 and got.K == 1
        same_table(got, composition(tab, n, mode, pos, r))
    for name, mode, r in (('keep', 0, None), ('last', 2, None), ('drop', 1, 0.6)):
        got = table_from_search(tab, n, pos_src=pos, pos_tgt=pos, radius=r, self_loops=name)
        want = composition(tab, n, mode, pos, r)
        same_table(got, want)
        (gp, ge), (wp, we) = got.reverse, want.reverse
        assert torch.equal(gp, wp) and int(gp[-1]) == got.n_edges > 0
        assert ge.shape == we.shape and torch.equal(ge[:got.n_edges], we[:got.n_edges])      # (the slots behind the edges are not written)


# ------------------------------------------------------------------------------------------------------------------ builders
SIZES = [700, 5, 300, 120]
K_B, R_B = 16, 0.15


@pytest.fixture(scope='module')
def clouds():
    """Three clouds of 700, 5 (below k: -1 columns) and 300 points and a fourth in which 20 points coincide (k of the others are at
    least as near as a point itself: rows that do not hold their own index).  No pair of one cloud is within rounding of R_B."""
    parts = [S.make_cloud(900 + s, n) + np.float32(3.0 * s) for s, n in enumerate(SIZES)]
    parts[3][40:60] = parts[3][40]
    pos = np.concatenate(parts).astype(np.float32)
    ids = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    p64, o = pos.astype(np.float64), 0
    for n in SIZES:                                              # every pair of a cloud: a superset of what any search returns
        i, j = np.divmod(np.arange(n * n), n)
        assert tie_free(p64[o:o + n], R_B, (i, j))
        o += n
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64, device=DEV)
    return t(pos), t(ids), ptr


def edges_table(edges, target_row, n_tgt, n_src):
    from crfconv_amd.graph import table_from_edges
    return table_from_edges(edges[target_row], edges[1 - target_row], n_tgt, n_src)


def attached(edges, target_row):
    from crfconv_amd.graph import attached_table
    tab = attached_table(edges, target_row)
    assert tab is not None and attached_table(edges, 1 - target_row) is None
    assert edges._crf_graph_table[0] is tab and edges._crf_graph_table[1] == edges._version
    return tab


@pytest.mark.parametrize('loop', [True, False])
def test_knn_graph_table(clouds, loop):
    from crfconv_amd.models import graph_ops
    pos, ids, ptr = clouds
    n = pos.shape[0]
    edges = graph_ops.knn_graph(pos, K_B, ids, loop=loop)
    want = edges_table(edges, 1, n, n)
    got = graph_ops.knn_graph_table(pos, K_B, ids, loop=loop)
    same_table(got, want)
    same_table(graph_ops.knn_graph_table(pos, K_B, loop=loop, ptr=ptr), got)
    same_table(attached(edges, 1), want)
    assert int((want.idx32[700:705] >= 0).sum(1).max()) == (5 if loop else 4)                      # the 5-point cloud: -1 columns
    own = (want.idx32 == torch.arange(n, device=DEV)[:, None]).any(1)
    if loop:
        assert 0 < int((~own).sum()) <= 20                       # coincident points crowd a row's own index out
        from crfconv_amd.graph import self_last_table
        last = self_last_table(got)
        assert last.K == K_B + 1 and self_last_table(got) is last
        loops = torch.arange(n, device=DEV)
        keep = edges[0] != edges[1]
        same_table(last, edges_table(torch.cat([edges[:, keep], torch.stack([loops, loops])], 1), 1, n, n))
    else:
        assert not bool(own.any())


@pytest.mark.parametrize('loop', [True, False])
def test_radius_graph_table(clouds, loop):
    from crfconv_amd.models import graph_ops
    pos, ids, ptr = clouds
    n = pos.shape[0]
    edges = graph_ops.radius_graph(pos, R_B, ids, loop=loop, max_num_neighbors=K_B)
    want = edges_table(edges, 1, n, n)
    got = graph_ops.radius_graph_table(pos, R_B, ids, loop=loop, max_num_neighbors=K_B)
    same_table(got, want)
    same_table(graph_ops.radius_graph_table(pos, R_B, loop=loop, max_num_neighbors=K_B, ptr=ptr), got)
    same_table(attached(edges, 1), want)
    deg = (want.idx32 >= 0).sum(1)
    uncut = (graph_ops.knn_graph_table(pos, K_B, ids, loop=loop).idx32 >= 0).sum(1)         # the same candidates without the cut
    assert int((deg == (1 if loop else 0)).sum()) > 0            # a row the radius leaves nothing (but itself)
    assert int(((deg == uncut) & (uncut >= 4)).sum()) > 0 and int((deg < uncut).sum()) > 0        # rows it leaves whole, rows it cuts


def test_knn_table_on_an_fps_subset(clouds):
    from crfconv_amd.models import graph_ops, point_conv as pc
    pos, ids, ptr = clouds
    pick = graph_ops.fps(pos, ids, ratio=0.25)
    sub_pos, sub_ids = pos[pick], ids[pick]
    sub_ptr = torch.zeros(len(SIZES) + 1, dtype=torch.int64, device=DEV)
    sub_ptr[1:] = torch.cumsum(torch.bincount(sub_ids, minlength=len(SIZES)), 0)
    edges = graph_ops.knn(pos, sub_pos, K_B, ids, sub_ids)       # [sub index; full index]
    want = edges_table(edges, 0, sub_pos.shape[0], pos.shape[0])
    got = graph_ops.knn_table(pos, sub_pos, K_B, ids, sub_ids)
    same_table(got, want)
    same_table(graph_ops.knn_table(pos, sub_pos, K_B, ptr_x=ptr, ptr_y=sub_ptr), got)
    same_table(attached(edges, 0), want)
    assert edges._crf_knn_table.K == K_B                         # the search's own table still rides along
    for method in ('knn', 'radius'):
        ei, p1, b1 = pc.build_bipartite_graph(pos, ids, 0.25, method=method, r=R_B, k=K_B)
        tab, p2, b2 = pc.build_bipartite_graph(pos, ids, 0.25, method=method, r=R_B, k=K_B, as_table=True)
        assert torch.equal(p1, p2) and torch.equal(b1, b2) and torch.equal(p1, sub_pos)
        same_table(tab, edges_table(ei, 1, sub_pos.shape[0], pos.shape[0]))
        same_table(attached(ei, 1), tab)
    row, col = edges
    keep = ((sub_pos[row] - pos[col]) ** 2).sum(1) <= R_B * R_B  # the framework mask the radius form used
    assert torch.equal(ei, torch.stack([col[keep], row[keep]]))
    for method in ('knn', 'radius'):
        ei = pc.build_graph(pos, ids, method=method, r=R_B, k=K_B)
        same_table(pc.build_graph(pos, ids, method=method, r=R_B, k=K_B, as_table=True), edges_table(ei, 1, pos.shape[0], pos.shape[0]))


def test_an_edge_tensor_written_in_place_loses_its_table(clouds):
    from crfconv_amd import ops
    from crfconv_amd.graph import attached_table
    from crfconv_amd.models import graph_ops
    from crfconv_amd.models.continuous_crf_conv import GuideGaussianCRFConv
    pos, ids, _ = clouds
    n = pos.shape[0]
    torch.manual_seed(3)
    layer = GuideGaussianCRFConv(16, 8, 8, radius=R_B, kernel_size=K_B, steps=2).to(DEV).eval()
    x, y = t(S.uniform(5, 'x', (n, 16))), t(S.uniform(5, 'y', (n, 8)))
    edges = graph_ops.radius_graph(pos, R_B, ids, loop=False, max_num_neighbors=K_B)
    with torch.no_grad():
        before = layer(x, y, pos, ids, edge_index=edges)
        assert attached_table(edges, 1) is not None
        edges[0, :50] = edges[1, :50].roll(7)                    # other sources for the first 50 edges
        assert attached_table(edges, 1) is None
        got = layer(x, y, pos, ids, edge_index=edges)
        ops.state.no_graph_tables = True
        try:
            want = layer(x, y, pos, ids, edge_index=edges.clone())
        finally:
            ops.state.no_graph_tables = False
    assert torch.equal(got, want) and not torch.equal(got, before)


# -------------------------------------------------------------------------------------------------------------------- layers
def three_ways(make_layer, inputs, graphs, call):
    """Forward and backward of one layer from the same state: given the table, given the edge tensor that carries it, and on the
    parent's path (ops.state.no_graph_tables: nothing attached, nothing consumed).  graphs(kind) -> the layer's graph argument."""
    from crfconv_amd import ops
    torch.manual_seed(11)
    proto = make_layer().to(DEV).train()
    runs = {}
    for kind in ('table', 'edges', 'parent'):
        ops.state.no_graph_tables = kind == 'parent'
        try:
            layer = copy.deepcopy(proto)
            ins = [v.clone().requires_grad_() for v in inputs]
            out = call(layer, ins, graphs(kind))
            (out * torch.linspace(0.5, 1.5, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
            runs[kind] = ([out.detach()] + [v.grad for v in ins], dict((k, p.grad) for k, p in layer.named_parameters()),
                          dict(layer.named_buffers()))
        finally:
            ops.state.no_graph_tables = False
    ref = runs['parent']
    assert all(g is not None for g in ref[1].values())
    for kind in ('table', 'edges'):
        got = runs[kind]
        for a, b in zip(got[0], ref[0]):
            assert torch.equal(a, b), kind
        for k in ref[1]:
            assert torch.equal(got[1][k], ref[1][k]), (kind, k)
        for k in ref[2]:
            assert torch.equal(got[2][k], ref[2][k]), (kind, k)


def test_point_conv_symmetric(clouds):
    from crfconv_amd.models import graph_ops
    from crfconv_amd.models.point_conv import DepthwiseSeparablePointConv
    pos, ids, _ = clouds
    x = t(S.uniform(21, 'x', (pos.shape[0], 12)))               # (d = 32, 64 below: the wide family; dW2 of d <= 16 goes through LDS
                                                                 # float atomics, whose order no table fixes -- test_gpu_model: 1e-6)

    def graphs(kind):
        return graph_ops.knn_graph_table(pos, K_B, ids, loop=True) if kind == 'table' else graph_ops.knn_graph(pos, K_B, ids, loop=True)
    three_ways(lambda: DepthwiseSeparablePointConv(12, 128), [x], graphs, lambda m, ins, g: m(ins[0], pos, g))


def test_point_conv_bipartite(clouds):
    from crfconv_amd.models import point_conv as pc
    pos, ids, _ = clouds
    x = t(S.uniform(22, 'x', (pos.shape[0], 32)))

    def graphs(kind):
        return pc.build_bipartite_graph(pos, ids, 0.25, method='knn', k=K_B, as_table=kind == 'table')
    three_ways(lambda: pc.DepthwiseSeparablePointConv(32, 256), [x], graphs, lambda m, ins, g: m(ins[0], (pos, g[1]), g[0]))


def test_guide_crf_conv(clouds):
    from crfconv_amd.models import graph_ops
    from crfconv_amd.models.continuous_crf_conv import GuideGaussianCRFConv
    pos, ids, _ = clouds
    n = pos.shape[0]
    x, y = t(S.uniform(23, 'x', (n, 32))), t(S.uniform(23, 'y', (n, 16)) * 0.3)

    def graphs(kind):
        build = graph_ops.radius_graph_table if kind == 'table' else graph_ops.radius_graph
        return build(pos, R_B, ids, loop=False, max_num_neighbors=K_B)
    three_ways(lambda: GuideGaussianCRFConv(32, 16, 16, radius=R_B, kernel_size=K_B, steps=2), [x, y], graphs,
               lambda m, ins, g: m(ins[0], ins[1], pos, ids, edge_index=g))

    def own_graph(m, ins, kind):                                 # the layer's own graph: an edge list, or (graph_tables) a table
        m.graph_tables = kind == 'table'
        return m(ins[0], ins[1], pos, ids)
    three_ways(lambda: GuideGaussianCRFConv(32, 16, 16, radius=R_B, kernel_size=K_B, steps=2), [x, y], lambda kind: kind, own_graph)


def test_sparse_continuous_crf_conv(clouds):
    """Its aggregating nodes are row 0 of the edge tensor: the orientation of `knn`, not of `knn_graph`, whose attached table it
    must not take."""
    from crfconv_amd.graph import attached_table, table_from_edges
    from crfconv_amd.models import graph_ops
    from crfconv_amd.models.continuous_crf_conv import ContinuousGaussianCRFConv
    pos, ids, _ = clouds
    n = pos.shape[0]
    x, y = t(S.uniform(24, 'x', (n, 32))), t(S.uniform(24, 'y', (n, 16)) * 0.3)

    def graphs(kind):
        return graph_ops.knn_table(pos, pos, K_B, ids, ids) if kind == 'table' else graph_ops.knn(pos, pos, K_B, ids, ids)
    make = lambda: ContinuousGaussianCRFConv(32, 16, None, 16, steps=2)
    three_ways(make, [x, y], graphs, lambda m, ins, g: m(ins[0], ins[1], pos, g))
    other = graph_ops.knn_graph(pos, K_B, ids, loop=True)        # targets in row 1
    assert attached_table(other, 1) is not None and attached_table(other, 0) is None
    three_ways(make, [x, y], lambda kind: table_from_edges(other[0], other[1], n, n) if kind == 'table' else other,
               lambda m, ins, g: m(ins[0], ins[1], pos, g))


def test_discrete_crf_conv(clouds):
    from crfconv_amd.models import DiscreteCRFConv, graph_ops
    pos, ids, _ = clouds
    n, L, D = pos.shape[0], 5, 6
    logit, f = t(S.uniform(25, 'l', (n, L), -2, 2)), t(S.uniform(25, 'f', (n, D), 0, 1))

    def graphs(kind):
        build = graph_ops.radius_graph_table if kind == 'table' else graph_ops.radius_graph
        return build(pos, R_B, ids, loop=False, max_num_neighbors=K_B)
    three_ways(lambda: DiscreteCRFConv(L, D, hidden_channels=16, num_kernels=3, radius=R_B, kernel_size=K_B, steps=2), [logit, f], graphs,
               lambda m, ins, g: torch.log(m(pos, torch.softmax(ins[0], -1), f=ins[1], batch=ids, edge_index=g)))


# ------------------------------------------------------------------------------------------------------------------- network
def test_crfsegnet_three_ways(monkeypatch):
    """CRFSegNet in training mode from one state: the parent's path, the default (edge lists that carry their tables) and
    graph_tables = True (no edge list, table_from_edges never reached, as many searches as the default)."""
    import crfconv_amd
    from crfconv_amd import _lib, graph, models, ops
    from crfconv_amd.models import continuous_crf_conv as ccc, point_conv as pc
    n0, n1 = 700, 500
    pos = t(np.concatenate([S.make_cloud(60, n0), S.make_cloud(61, n1)]))
    batch = t(np.concatenate([np.zeros(n0, np.int64), np.ones(n1, np.int64)]))
    data = crfconv_amd.Data(pos=pos, x=t(S.uniform(60, 'f', (n0 + n1, 6))), batch=batch)
    label = t(S.integers(60, 'y', (n0 + n1,), 0, 5))
    torch.manual_seed(5)
    proto = models.CRFSegNet(6, 5, steps=2).to(DEV).train()
    seen = []
    real = _lib.call

    def call(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)

    def refuse(*a, **k):
        raise AssertionError('table_from_edges reached with graph_tables = True')

    runs = {}
    for kind in ('parent', 'default', 'tables'):
        net = copy.deepcopy(proto)
        del seen[:]
        with monkeypatch.context() as mp:
            mp.setattr(ops.state, 'no_graph_tables', kind == 'parent')
            if kind == 'tables':
                pc.use_graph_tables(net)
                for mod in (graph, pc, ccc):
                    mp.setattr(mod, 'table_from_edges', refuse)
            logp = net(data)
            torch.nn.functional.nll_loss(logp, label).backward()
        runs[kind] = (logp.detach(), dict((k, p.grad) for k, p in net.named_parameters()), dict(net.named_buffers()),
                      seen.count('crfconv_knn_segments_dev'), seen.count('crfconv_graph_table'))
    ref = runs['parent']
    assert ref[4] == 0 and ref[3] > 0
    assert any('running_mean' in k for k in ref[2]) and all(g is not None for g in ref[1].values())
    for kind in ('default', 'tables'):
        got = runs[kind]
        assert torch.equal(got[0], ref[0]), kind
        for k in ref[1]:
            assert torch.equal(got[1][k], ref[1][k]), (kind, k)
        for k in ref[2]:
            assert torch.equal(got[2][k], ref[2][k]), (kind, k)
    assert runs['tables'][3] == runs['default'][3] == ref[3]
    assert runs['tables'][4] > 0 and runs['default'][4] > 0


# ----------------------------------------------------------------------------------- dense tables through the batched narrowing
def narrowed(idx, n_src):
    """numpy restatement of the narrowing: cloud b's local id j -> b n_src + j, columns 1 .. K-1 of a row ascending (K <= 64: wider
    rows keep their order); the local ids as uint16."""
    B, n, K = idx.shape
    loc = idx.copy()
    if 1 < K <= 64:
        loc[:, :, 1:] = np.sort(loc[:, :, 1:], axis=2)
    glob = (loc + (np.arange(B, dtype=np.int64) * n_src)[:, None, None]).reshape(B * n, K)
    return glob.astype(np.int32), loc.reshape(B * n, K).astype(np.uint16)


@pytest.mark.parametrize('K,n_src', [(16, 1000), (1, 1000), (65, 1000), (24, 70000), (5, 300)])
def test_dense_tables_through_the_batched_narrowing(K, n_src):
    from crfconv_amd.graph import NeighborTable
    B, n = 3, 301                                                # 903 rows: a last partial workgroup
    idx = S.integers(70 + K, 'idx', (B, n, K), 0, n_src).astype(np.int64)
    tab = NeighborTable(t(idx), n_src)
    i32, i16 = narrowed(idx, n_src)
    assert tuple(tab.idx32.shape) == (B * n, K) and np.array_equal(tab.idx32.cpu().numpy(), i32)
    if n_src <= 65536 and K % 8 == 0:
        assert np.array_equal(tab.idx16.cpu().numpy().view(np.uint16), i16)
    else:
        assert tab.idx16 is None
    idx2 = S.integers(170 + K, 'idx', (B, n, K), 0, n_src).astype(np.int64)
    tab.refresh_(t(idx2))                                        # the unbatched branch of refresh_
    assert np.array_equal(tab.idx32.cpu().numpy(), narrowed(idx2, n_src)[0])
    bad = idx.copy()
    bad[1, 7, K - 1], bad[2, 300, 0] = n_src, -1
    with pytest.raises(IndexError, match='2 neighbour indices outside'):
        NeighborTable(t(bad), n_src)
