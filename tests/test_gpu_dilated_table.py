"""-m gpu: randomly dilated kNN graphs as neighbour tables from one finishing launch (csrc/graph_table.hip: graph_table_dilated_kernel,
graph.table_from_search_dilated, graph_ops.knn_dilated_table, the draw= forms of the builders) against the numpy restatement of the
draw (dilated_restatement.py): the table must be the one graph.table_from_edges groups out of the restatement's edge list --
torch.equal, no tolerance: the draw is integer arithmetic."""
import copy

import numpy as np
import pytest
import torch

import _seeded as S
import dilated_restatement as R
from test_gpu_graph_table import same_table, synthetic, t

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 20250                # the seed of test_host_dilated_table.py's uniformity case
MODES = ('keep', 'drop', 'last')


def counter_word(value=0):
    return torch.full((1,), value, dtype=torch.int64, device=DEV)


def want_table(picks, mode, n_src):
    from crfconv_amd.graph import table_from_edges
    row, col = R.edges_of(picks, mode)
    return table_from_edges(t(row), t(col), len(picks), n_src), row


def full_width(tab, counts, want, k_out):
    """The read_counts=False form: the table at its full width -- the narrowed one, then -1 -- and the counts on the device."""
    assert tuple(tab.idx32.shape) == (want.n_tgt, k_out) and tab.padded and tab.B == 1 and tab.n_src == want.n_src
    if want.n_edges:
        assert torch.equal(tab.idx32[:, :want.K], want.idx32) and bool((tab.idx32[:, want.K:] == -1).all())
        assert counts.tolist() == [want.n_edges, want.K]
    else:
        assert bool((tab.idx32 == -1).all()) and counts.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ the kernel against the restatement
def search_like(n, K, k, seed):
    """[n, K] rows as a search leaves them: a valid prefix (the row itself first, then other rows, some twice), -1 behind it; prefix
    lengths K, 0, 1, k - 1 (have < k_pick), k and random ones."""
    rng = np.random.default_rng(seed)
    tab = ((np.arange(n)[:, None] + rng.integers(1, 12, (n, K)).cumsum(1) // 2) % n).astype(np.int32)
    tab[:, 0] = np.arange(n)
    have = rng.integers(0, K + 1, n)
    for r, h in enumerate((K, 0, 1, k - 1, k)):
        have[r::9] = h
    tab[np.arange(K)[None, :] >= have[:, None]] = -1
    return tab


@pytest.mark.parametrize('K,k', [(2, 1), (3, 2), (16, 16), (17, 4), (32, 16), (33, 8), (64, 16), (64, 32), (64, 63)])
def test_kernel_equals_the_restatement(K, k):
    """Both sides of every lane-group width (W = next power of two >= max(K, K_out): 2 .. 64, K_out = 64 in mode 2 of (64, 63)), one
    row, a last partial workgroup, all self modes, search-like and hole-ridden tables."""
    from crfconv_amd.graph import table_from_search_dilated
    for n in (1, 257, 1005):
        for kind, tab_np in (('search', search_like(n, K, k, 31 * K + k + n)), ('holes', synthetic(n, K, 100 * K + k + n))):
            tab, counter, salt = t(tab_np), counter_word(3), K + n
            picks = R.picks_of(tab_np, n, k, SEED, 3, salt)
            valid = ((tab_np >= 0) & (tab_np < n)).sum(1)
            assert [p.size for p in picks] == np.minimum(valid, k).tolist()
            if n > 1:
                assert (valid == 0).any()                        # rows without a neighbour
            if n > 1 and kind == 'search':
                assert (valid == 1).any() and (valid >= k).any() and (k == 1 or (valid == k - 1).any())      # have = 1, >= k, < k
            for mode, name in enumerate(MODES):
                if k + (mode == 2) > 64:
                    continue
                want, row = want_table(picks, mode, n)
                got = table_from_search_dilated(tab, n, k, seed=SEED, counter=counter, salt=salt, self_loops=name)
                same_table(got, want)
                assert got.n_edges == row.size
                full_width(*table_from_search_dilated(tab, n, k, seed=SEED, counter=counter, salt=salt, self_loops=name, read_counts=False),
                           want, k + (mode == 2))
    # mode 0 over another number of sources (a bipartite table): entries past n_src are holes
    tab_np = synthetic(257, K, 900 + K)
    got = table_from_search_dilated(t(tab_np), 200, k, seed=SEED, counter=counter_word(0), salt=0)
    same_table(got, want_table(R.picks_of(tab_np, 200, k, SEED, 0, 0), 0, 200)[0])
    with pytest.raises(ValueError):
        table_from_search_dilated(t(tab_np), 200, k, seed=SEED, counter=counter_word(0), salt=0, self_loops='drop')


def test_kernel_walks_on_over_the_tiles_and_draws_uniformly():
    """4100 tiles of 4 rows for 1024 workgroups (several trips, the last one partial); the first 4096 rows are full, so their slot
    counts are the ones the host test bounds: within 6 sqrt(65536 (1/64) (63/64)) = 190.5 of 1024."""
    from crfconv_amd.graph import table_from_search_dilated
    n, K, k = 16399, 64, 16
    tab_np = (np.arange(n)[:, None] * 64 + np.arange(K)[None, :]).astype(np.int32)       # entry = 64 row + column: the pick names its slot
    tab_np[4096:] = synthetic(n - 4096, K, 77)
    n_src = 64 * n
    got = table_from_search_dilated(t(tab_np), n_src, k, seed=SEED, counter=counter_word(0), salt=0)
    picks = R.picks_of(tab_np, n_src, k, SEED, 0, 0)
    same_table(got, want_table(picks, 0, n_src)[0])
    slots = (got.idx32[:4096].long() % 64).flatten()
    count = torch.bincount(slots, minlength=64).cpu().numpy()
    assert count.sum() == 65536 and np.abs(count - 1024).max() <= 6.0 * np.sqrt(65536 * (1 / 64) * (63 / 64))


def test_no_edge_at_all():
    from crfconv_amd.graph import table_from_search_dilated
    tab = torch.full((300, 8), -1, dtype=torch.int32, device=DEV)
    tab[::2] = 300
    got = table_from_search_dilated(tab, 300, 4, seed=1, counter=counter_word(), salt=0, self_loops='drop')
    assert tuple(got.idx32.shape) == (300, 1) and got.n_edges == 0 and got.K == 1 and bool((got.idx32 == -1).all())
    own = torch.arange(300, dtype=torch.int32, device=DEV)[:, None].repeat(1, 8)          # rows that hold only themselves
    got = table_from_search_dilated(own, 300, 4, seed=1, counter=counter_word(), salt=0, self_loops='drop')
    assert tuple(got.idx32.shape) == (300, 1) and got.n_edges == 0
    got = table_from_search_dilated(own, 300, 4, seed=1, counter=counter_word(), salt=0, self_loops='last')
    assert tuple(got.idx32.shape) == (300, 1) and got.n_edges == 300 and torch.equal(got.idx32[:, 0], own[:, 0])


# ------------------------------------------------------------------------------------------------------------------------ keys
def test_keys():
    from crfconv_amd.graph import table_from_search_dilated
    from crfconv_amd.models import graph_ops
    n, K, k = 1005, 32, 8
    tab_np = search_like(n, K, k, 5)
    tab = t(tab_np)

    def run(seed, counter, salt):
        return table_from_search_dilated(tab, n, k, seed=seed, counter=counter_word(counter), salt=salt).idx32
    base = run(11, 4, 2)
    assert torch.equal(base, run(11, 4, 2))
    for other in ((12, 4, 2), (11, 5, 2), (11, 4, 3), (11 + (1 << 40), 4, 2)):
        assert not torch.equal(base, run(*other)), other
    assert torch.equal(base, run(11 + (1 << 64), 4, 2))                                    # the seed's low 64 bits
    # a DilationDraw: the salts count up on the host, step() moves the device word
    draw, twin = graph_ops.DilationDraw(11, DEV), graph_ops.DilationDraw(11, DEV)
    pos = t(S.make_cloud(8, 400))
    idx = graph_ops._knn_table(pos, pos, 32, None, None).cpu().numpy()
    for counter in (0, 1):
        for salt in (2 * counter, 2 * counter + 1):
            got = graph_ops.knn_dilated_table(pos, pos, 8, 4, draw=draw)
            same_table(got, want_table(R.picks_of(idx, 400, 8, 11, counter, salt), 0, 400)[0])
            same_table(graph_ops.knn_dilated_table(pos, pos, 8, 4, draw=twin), got)
        draw.step()
        twin.step()
    assert draw.counter.tolist() == [2]
    with pytest.raises(ValueError):
        graph_ops.knn_dilated_table(pos, pos, 13, 5, draw=draw)


# -------------------------------------------------------------------------------------------------------------------- builders
SIZES = [700, 5, 300]
K_B, D_B = 8, 4


@pytest.fixture(scope='module')
def clouds():
    """Three clouds of 700, 5 (fewer than k * d and than k points) and 300 points."""
    pos = np.concatenate([S.make_cloud(900 + s, n) + np.float32(3.0 * s) for s, n in enumerate(SIZES)]).astype(np.float32)
    ids = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64, device=DEV)
    return t(pos), t(ids), ptr


@pytest.mark.parametrize('loop', [True, False])
def test_build_graph_with_a_draw(clouds, loop, monkeypatch):
    from crfconv_amd.models import graph_ops, point_conv as pc
    pos, ids, _ = clouds
    n = pos.shape[0]
    idx = graph_ops._knn_table(pos, pos, K_B * D_B, ids, ids).cpu().numpy()
    assert idx.shape == (n, 32) and (idx[700:705, 5:] == -1).all() and (idx[700:705, :5] >= 700).all()
    draw = graph_ops.DilationDraw(21, DEV)
    for salt in (0, 1):                                          # every graph takes the draw's next salt
        got = pc.build_graph(pos, ids, method='knn', k=K_B, dilation=D_B, loop=loop, as_table=True, draw=draw)
        picks = R.picks_of(idx, n, K_B, 21, 0, salt)
        assert [p.size for p in picks[700:705]] == [5] * 5
        same_table(got, want_table(picks, 0 if loop else 1, n)[0])
    with pytest.raises(ValueError):
        pc.build_graph(pos, ids, method='knn', k=K_B, dilation=D_B, loop=loop, draw=draw)
    # a draw changes nothing for the graphs that are not dilated kNN graphs
    same_table(pc.build_graph(pos, ids, method='knn', k=K_B, loop=loop, as_table=True, draw=draw),
               pc.build_graph(pos, ids, method='knn', k=K_B, loop=loop, as_table=True))
    # without a draw the picks are torch.randint's, on an edge list
    calls = []
    real = graph_ops.knn_dilated
    monkeypatch.setattr(graph_ops, 'knn_dilated', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for as_table in (True, False):
        pc.build_graph(pos, ids, method='knn', k=K_B, dilation=D_B, loop=loop, as_table=as_table)
    assert len(calls) == 2
    pc.build_graph(pos, ids, method='knn', k=K_B, dilation=D_B, loop=loop, as_table=True, draw=draw)
    assert len(calls) == 2


def test_build_bipartite_graph_with_a_draw(clouds):
    from crfconv_amd.models import graph_ops, point_conv as pc
    pos, ids, ptr = clouds
    n = pos.shape[0]
    pick = graph_ops.fps(pos, ids, ratio=0.25)
    sub_pos, sub_ids = pos[pick], ids[pick]
    idx = graph_ops._knn_table(pos, sub_pos, K_B * D_B, ids, sub_ids).cpu().numpy()
    got, p1, b1 = pc.build_bipartite_graph(pos, ids, 0.25, method='knn', k=K_B, dilation=D_B, as_table=True,
                                           draw=graph_ops.DilationDraw(22, DEV))
    assert torch.equal(p1, sub_pos) and torch.equal(b1, sub_ids)
    picks = R.picks_of(idx, n, K_B, 22, 0, 0)
    assert [p.size for p in picks[175:177]] == [5, 5] and sub_ids[175:177].tolist() == [1, 1]
    same_table(got, want_table(picks, 0, n)[0])
    # the ptr form, handed a draw in the same state
    tab, p2, sub_ptr = pc.build_bipartite_graph(pos, None, 0.25, method='knn', k=K_B, dilation=D_B, as_table=True, ptr=ptr,
                                                draw=graph_ops.DilationDraw(22, DEV))
    same_table(tab, got)
    assert torch.equal(p2, sub_pos) and sub_ptr.tolist() == [0, 175, 177, 252]
    with pytest.raises(ValueError):
        pc.build_bipartite_graph(pos, None, 0.25, method='knn', k=K_B, dilation=D_B, as_table=True, ptr=ptr)
    with pytest.raises(ValueError):
        pc.build_bipartite_graph(pos, ids, 0.25, method='knn', k=K_B, dilation=D_B, draw=graph_ops.DilationDraw(22, DEV))


# --------------------------------------------------------------------------------------------------------------------- capture
def test_capture_and_replay(clouds):
    """knn_dilated_table in its ptr form with read_counts=False makes no host read: captured, every replay draws by the counter word
    as it stands then."""
    from crfconv_amd.models import graph_ops
    pos, ids, ptr = clouds
    n = pos.shape[0]
    pick, sub_ptr = graph_ops.fps_segments(pos, ptr, 0.25)
    sub_pos = pos[pick]
    idx = graph_ops._knn_table(pos, sub_pos, K_B * D_B, None, None, ptr, sub_ptr).cpu().numpy()
    draw = graph_ops.DilationDraw(23, DEV)

    def build():
        return graph_ops.knn_dilated_table(pos, sub_pos, K_B, D_B, draw=draw, ptr_x=ptr, ptr_y=sub_ptr, read_counts=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        build()                                                  # salt 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tab, counts = build()                                    # salt 1
    seen = []
    for counter in (0, 1, 2):
        graph.replay()
        want = want_table(R.picks_of(idx, n, K_B, 23, counter, 1), 0, n)[0]
        full_width(tab, counts, want, K_B)
        seen.append(tab.idx32.clone())
        draw.step()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# -------------------------------------------------------------------------------------------------------------------- networks
def part_data(n):
    import crfconv_amd
    pos = t(np.concatenate([S.make_cloud(70, n), S.make_cloud(71, n)]))
    feat = t(S.uniform(70, 'f', (2 * n, 6), 0, 1))
    batch = t(np.repeat(np.arange(2, dtype=np.int64), n))
    return crfconv_amd.Data(pos=pos, norm=feat[:, 3:], x=feat, batch=batch, category=t(np.array([3, 9], dtype=np.int64)))


@pytest.mark.parametrize('name', ['CRFSegNet_Part', 'DualCRFSegNet'])
def test_networks_draw_on_the_device(name, monkeypatch):
    """Two clouds of 512 points: k * d <= 64 at every level; the coarse levels hold fewer points than that, and the search is then as
    wide as the level.  Forward and backward in training mode without knn_dilated and without table_from_edges."""
    from crfconv_amd import graph, models
    from crfconv_amd.models import continuous_crf_conv as ccc, graph_ops, point_conv as pc
    data = part_data(512)
    label = t(S.integers(70, 'y', (1024,), 0, 5))
    torch.manual_seed(5)
    proto = getattr(models, name)(6, 5, steps=1).to(DEV).train()
    assert all(k * d <= 64 for k, d in zip(proto.feature.kernel_size, proto.feature.dilation)) and max(proto.feature.dilation) > 1
    calls = []

    def counted(fn, tag):
        return lambda *a, **k: (calls.append(tag), fn(*a, **k))[1]
    monkeypatch.setattr(graph_ops, 'knn_dilated', counted(graph_ops.knn_dilated, 'knn_dilated'))
    for mod in (graph, pc, ccc):
        monkeypatch.setattr(mod, 'table_from_edges', counted(mod.table_from_edges, 'table_from_edges'))

    def run(seed):
        net = pc.use_device_dilation(copy.deepcopy(proto), seed=seed)
        assert net.feature.graph_tables and net.feature.dilation_draw.seed == seed
        out = net(data)
        outs = out if isinstance(out, tuple) else (out,)
        for o in outs:
            assert tuple(o.shape) == (1024, 5) and bool(torch.isfinite(o).all())
            assert float((o.detach().exp().sum(-1) - 1).abs().max()) < 1e-4                       # log-probabilities
        sum(torch.nn.functional.nll_loss(o, label) for o in outs).backward()
        for k, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        return [o.detach() for o in outs]
    a, b, c = run(3), run(3), run(4)
    assert calls == []
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(torch.equal(x, y) for x, y in zip(a, c))
    assert proto.feature.dilation_draw is None and not proto.feature.graph_tables
    # the same network without the device draw goes through knn_dilated (graph_tables alone: on an edge list, then grouped)
    pc.use_graph_tables(copy.deepcopy(proto))(data)
    assert 'knn_dilated' in calls and 'table_from_edges' in calls
