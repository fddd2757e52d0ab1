"""-m gpu: csrc/pool.hip kernel by kernel -- neighbour max-pool (plain and BatchNorm-affine), row gather, the residual join and
LeakyReLU -- against float64 references written here in numpy / torch on the CPU.  Every reference is driven by the table AS THE
DEVICE HOLDS IT (tab.idx32 read back): "column order" below is the kernel's order, i.e. columns 1.. re-sorted by source id for a
dense table, a target's edges in their input order for a table built from an edge list.

Sites that say "exact" compare with array_equal / torch.equal; the others state their bound at the assert_close call."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, assert_close, t

pytestmark = pytest.mark.gpu


@pytest.fixture
def big_forms_from_4096(monkeypatch):
    """As in test_gpu_model.py: the row-streaming (big-level) forms from 4 096 rows on, so that 4 100 rows reach them."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'mfma_min_rows', 4096)


# ------------------------------------------------------------------ references and helpers
def device_rows(tab):
    """The table as the kernels read it: int64 [m_tgt, K] GLOBAL source rows, -1 = no neighbour."""
    return tab.idx32.cpu().numpy().astype(np.int64)


def ref_pool(x64, rows, gout64=None, a=None, b=None):
    """float64 max over a row's valid columns of (a x + b); the FIRST column that attains the max wins (numpy's argmax), a row
    without a valid column gives 0 and arg -1.  Returns (out, arg, dx): dx scatters gout to the winning edge alone."""
    valid = rows >= 0
    v = x64[np.where(valid, rows, 0)]                                   # [m_tgt, K, C]
    if a is not None:
        v = a * v + b
    v = np.where(valid[:, :, None], v, -np.inf)
    arg = v.argmax(1)
    out = np.take_along_axis(v, arg[:, None, :], 1)[:, 0, :]
    empty = ~valid.any(1)
    out[empty] = 0.0
    arg[empty] = -1
    dx = None
    if gout64 is not None:
        dx = np.zeros_like(x64)
        src = np.take_along_axis(rows, np.maximum(arg, 0), 1)           # [m_tgt, C] winning source row
        sel = arg >= 0
        cols = np.broadcast_to(np.arange(x64.shape[1]), arg.shape)
        np.add.at(dx, (src[sel], cols[sel]), gout64[sel])
    return out, arg, dx


def ref_pool_edges(x64, tgt, src, n_tgt, gout64):
    """The same over an EDGE LIST, edge by edge in input order (a strict > keeps the first edge of a target that attains the max)."""
    C = x64.shape[1]
    out = np.full((n_tgt, C), -np.inf)
    win = np.full((n_tgt, C), -1, dtype=np.int64)
    for e in range(len(tgt)):
        v = x64[src[e]]
        m = v > out[tgt[e]]
        out[tgt[e]][m] = v[m]
        win[tgt[e]][m] = e
    out[win < 0] = 0.0
    dx = np.zeros_like(x64)
    for i, c in zip(*np.nonzero(win >= 0)):
        dx[src[win[i, c]], c] += gout64[i, c]
    return out, dx


def near_tie_mask(x64, rows, a=None, b=None):
    """(target, channel) entries whose two largest float64 candidates differ by less than 1e-5 max(1, |max|): there an fp32 and an
    fp64 argmax may legitimately disagree.  From the reference alone."""
    valid = rows >= 0
    v = x64[np.where(valid, rows, 0)]
    if a is not None:
        v = a * v + b
    v = np.sort(np.where(valid[:, :, None], v, -np.inf), 1)
    if v.shape[1] < 2:
        return np.zeros((v.shape[0], v.shape[2]), dtype=bool)
    top, second = v[:, -1, :], v[:, -2, :]
    with np.errstate(invalid='ignore'):
        gap = np.where(np.isfinite(second), top - second, np.inf)
    return gap < 1e-5 * np.maximum(1.0, np.abs(np.where(np.isfinite(top), top, 0.0)))


def poison(shape):
    """A freed device block of this shape full of NaN: the torch.empty the backward allocates next tends to reuse it, so a gradient
    row that the kernel leaves unwritten shows as NaN, not as a zero that happened to lie there."""
    torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()


def run_pool(x, tab, gout):
    """ops.neighbor_maxpool forward + backward on float32 host arrays -> (out, dx) as float64 numpy."""
    from crfconv_amd import ops
    xd = t(x).requires_grad_(True)
    out = ops.neighbor_maxpool(xd, tab)
    poison(tuple(xd.shape))
    out.backward(t(gout))
    return out.detach().cpu().double().numpy(), xd.grad.cpu().double().numpy()


def dense_table(rng, B, n_tgt, n_src, K, lo=0, hi=None):
    from crfconv_amd.graph import NeighborTable
    idx = rng.integers(lo, n_src if hi is None else hi, (B, n_tgt, K))
    return NeighborTable(t(idx), n_src), idx


def edge_table(rng, n_tgt, n_src, degrees):
    """A padded table from a shuffled edge list whose per-target in-degrees are drawn from `degrees` (each value occurs)."""
    from crfconv_amd.graph import table_from_edges
    deg = rng.choice(np.asarray(degrees), n_tgt)
    deg[:len(degrees)] = degrees
    deg[-1] = 0                                                          # the last target (the tail of the last workgroup) has no edge
    tgt = np.repeat(np.arange(n_tgt), deg)
    src = rng.integers(0, n_src, tgt.size)
    perm = rng.permutation(tgt.size)
    tgt, src = tgt[perm], src[perm]
    tab = table_from_edges(t(tgt), t(src), n_tgt, n_src)
    assert tab.padded and tab.K == max(degrees) and tab.n_edges == tgt.size
    return tab, tgt, src, deg


# ------------------------------------------------------------------ 1. max-pool over table shapes
@pytest.mark.parametrize('K,C', [(1, 4), (3, 8), (4, 36), (5, 132), (7, 8), (16, 4), (24, 132), (33, 36), (5, 6), (16, 132)])
def test_maxpool_table_shapes(K, C):
    """K % 4 != 0 takes the tail guard of the four-neighbour trip, a K that is no power of two the integer divide of the backward's
    edge id -> (row, column); C = 6 goes through the channel-padding wrapper.  Forward exact, backward to 1e-6 of the float64 scatter."""
    B, n_src, n_tgt = 2, 300, 77
    rng = np.random.default_rng(1000 * K + C)
    tab, _ = dense_table(rng, B, n_tgt, n_src, K)
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    rows = device_rows(tab)
    assert rows.shape == (B * n_tgt, K) and rows.min() >= 0
    ref, _, dref = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert_close(dx, dref, 1e-6, 'maxpool grad')
    unused = np.setdiff1d(np.arange(B * n_src), rows)
    assert np.all(dx[unused] == 0.0)


def test_maxpool_duplicate_source_in_one_row():
    """A row that names one source twice: both columns lead to the same source row, whose gradient gets the entry once."""
    B, n_src, n_tgt, K, C = 2, 300, 77, 16, 8
    rng = np.random.default_rng(77)
    tab, _ = dense_table(rng, B, n_tgt, n_src, K)
    rows = device_rows(tab)
    dup = np.array([len(np.unique(r)) < K for r in rows])
    assert dup.any()
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    for i in np.nonzero(dup)[0][:8]:                                     # ... and the doubled source IS the maximum of some channels
        r = rows[i]
        j = [v for v in r if (r == v).sum() > 1][0]
        x[j, :4] = 9.0 + i
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    ref, _, dref = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert_close(dx, dref, 1e-6, 'maxpool grad')


@pytest.mark.parametrize('K', [5, 16])
def test_maxpool_half_used_sources_get_exact_zeros(K):
    """Indices from the first 150 rows of each cloud only: zero in-degree for the other 150, whose gradient rows (dx is torch.empty)
    must be written as exact zeros."""
    B, n_src, n_tgt, C = 2, 300, 77, 36
    rng = np.random.default_rng(150 + K)
    tab, _ = dense_table(rng, B, n_tgt, n_src, K, hi=150)
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    rows = device_rows(tab)
    ref, _, dref = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert_close(dx, dref, 1e-6, 'maxpool grad')
    dx = dx.reshape(B, n_src, C)
    assert np.array_equal(dx[:, 150:], np.zeros((B, 150, C)))
    assert np.abs(dx[:, :150]).max() > 0


def test_maxpool_hub_source():
    """Source 0 in every row (column 0 keeps its place): a reverse row of >= 1031 edges, no multiple of 4."""
    from crfconv_amd.graph import NeighborTable
    n_src, n_tgt, K, C = 64, 1031, 5, 8
    rng = np.random.default_rng(1031)
    idx = rng.integers(0, n_src, (1, n_tgt, K))
    idx[:, :, 0] = 0
    tab = NeighborTable(t(idx), n_src)
    rows = device_rows(tab)
    indeg = int((rows == 0).sum())
    assert np.all(rows[:, 0] == 0) and indeg >= 1031 and indeg % 4 != 0
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    x[0, :4] = 1.0                                                       # the hub wins often in these channels
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    ref, arg, dref = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))
    assert (np.take_along_axis(rows, arg, 1) == 0).sum() > 1000          # ... so its gradient row sums many entries
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert_close(dx[0], dref[0], 1e-6, 'hub row')
    assert_close(dx, dref, 1e-6, 'maxpool grad')


@pytest.mark.parametrize('K', [7, 16])
def test_maxpool_ties_go_to_the_first_column(K):
    """x from {-2 .. 2}: most rows have several columns -- of distinct sources -- at the maximum.  The first of them in device order
    gets the whole gradient; gradients are small integers, so every sum is exact and forward and dx equal the reference bit for bit."""
    B, n_src, n_tgt, C = 2, 300, 77, 8
    rng = np.random.default_rng(70 + K)
    tab, _ = dense_table(rng, B, n_tgt, n_src, K)
    x = rng.integers(-2, 3, (B * n_src, C)).astype(np.float32)
    gout = rng.integers(-3, 4, (B * n_tgt, C)).astype(np.float32)
    rows = device_rows(tab)
    x64 = x.astype(np.float64)
    ref, arg, dref = ref_pool(x64, rows, gout.astype(np.float64))
    cand = x64[rows]                                                     # a tie between two DIFFERENT sources, the first not in the last column
    tied = (cand == ref[:, None, :]) & (rows[:, :, None] != np.take_along_axis(rows, arg, 1)[:, None, :])
    assert tied.any(1).mean() > 0.3
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert np.array_equal(dx, dref)


# ------------------------------------------------------------------ 2. padded tables
@pytest.mark.parametrize('C', [4, 36])
def test_maxpool_padded_table_against_the_edge_list(C):
    """graph.table_from_edges with in-degrees from {0, 1, 2, 5}: -1 slots are skipped, a target without an edge outputs exactly 0 and
    sends no gradient.  The reference runs over the EDGE LIST, not over the padded table."""
    n_tgt, n_src = 257, 190
    rng = np.random.default_rng(257 + C)
    tab, tgt, src, deg = edge_table(rng, n_tgt, n_src, (0, 1, 2, 5))
    rows = device_rows(tab)
    assert rows.shape == (n_tgt, 5) and np.array_equal((rows >= 0).sum(1), deg) and (deg == 0).sum() > 10
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    ref, dref = ref_pool_edges(x.astype(np.float64), tgt, src, n_tgt, gout.astype(np.float64))
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert np.array_equal(out[deg == 0], np.zeros(((deg == 0).sum(), C)))
    assert_close(dx, dref, 1e-6, 'maxpool grad')
    assert np.all(dx[np.setdiff1d(np.arange(n_src), src)] == 0.0)
    ref2, _, dref2 = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))      # the two references agree with each other
    assert np.array_equal(ref, ref2) and np.allclose(dref, dref2, rtol=0, atol=1e-12)


def test_maxpool_table_without_edges():
    """E = 0: one column of -1.  crfconv_reverse_csr counts entries < 0 in a bin past the last source row and its fill pass skips them
    (csrc/graph.hip: rev_count_kernel / rev_fill_kernel), so every reverse row is empty: output and dx are all zeros."""
    from crfconv_amd.graph import table_from_edges
    n_tgt, n_src, C = 257, 190, 8
    none = torch.empty(0, dtype=torch.long, device=DEV)
    tab = table_from_edges(none, none, n_tgt, n_src)
    assert tab.padded and tab.K == 1 and tab.n_edges == 0 and bool((tab.idx32 == -1).all())
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, np.zeros((n_tgt, C)))
    assert np.array_equal(dx, np.zeros((n_src, C)))
    rev_ptr, _ = tab.reverse
    assert int(rev_ptr.abs().max()) == 0


def test_maxpool_padded_table_ties_first_valid_column():
    """Quantised x on the padded table: leading real entries, trailing -1s; the first VALID column at the maximum gets the gradient."""
    n_tgt, n_src, C = 257, 190, 8
    rng = np.random.default_rng(2570)
    tab, tgt, src, deg = edge_table(rng, n_tgt, n_src, (0, 1, 2, 5))
    rows = device_rows(tab)
    assert np.all((rows[:, 1:] >= 0) <= (rows[:, :-1] >= 0))             # real entries lead, -1s trail
    x = rng.integers(-2, 3, (n_src, C)).astype(np.float32)
    gout = rng.integers(-3, 4, (n_tgt, C)).astype(np.float32)
    ref, dref = ref_pool_edges(x.astype(np.float64), tgt, src, n_tgt, gout.astype(np.float64))
    ref2, arg, dref2 = ref_pool(x.astype(np.float64), rows, gout.astype(np.float64))
    assert np.array_equal(ref, ref2) and np.array_equal(dref, dref2)
    cand = np.where((rows >= 0)[:, :, None], x.astype(np.float64)[np.maximum(rows, 0)], -np.inf)
    assert ((cand == ref[:, None, :]).sum(1)[deg == 5] > 1).mean() > 0.3 # ties are common among the full rows
    out, dx = run_pool(x, tab, gout)
    assert np.array_equal(out, ref)
    assert np.array_equal(dx, dref)


# ------------------------------------------------------------------ 3. gather rows
@pytest.mark.parametrize('C', [4, 132, 6])
@pytest.mark.parametrize('form', ['random', 'hub'])
def test_gather_rows_forms(form, C):
    """ops.gather_rows (nearest up-sampling) on a random up-index and on one whose whole first cloud names a single source (a reverse
    row of 1031 edges): forward exact, backward to 1e-6 of the float64 scatter, unreferenced sources exactly 0.
    gather_rows_bwd_kernel sums a reverse row 64 edges at a time in float and adds those sums in double: one float running sum over
    the 1031 edges of the hub row (replayed in numpy float32 on this test's data: 1.8e-7 for C = 4, 4.7e-7 for C = 132, 1.35e-6 for
    C = 6) missed 1e-6 at C = 6; the blocked sum replayed the same way gives 3.8e-8, 1.3e-7 and 4.6e-8."""
    from crfconv_amd import ops
    from crfconv_amd.graph import NeighborTable
    B, n_src = 2, 300
    n_tgt = 1031 if form == 'hub' else 77
    rng = np.random.default_rng(C + (500 if form == 'hub' else 0))
    up = rng.integers(0, n_src, (B, n_tgt, 1))
    if form == 'hub':
        up[0] = 17
    tab = NeighborTable(t(up), n_src)
    rows = device_rows(tab)[:, 0]
    assert np.array_equal(rows, (up[:, :, 0] + np.arange(B)[:, None] * n_src).reshape(-1))
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    xd = t(x).requires_grad_(True)
    out = ops.gather_rows(xd, tab)
    poison(tuple(xd.shape))
    out.backward(t(gout))
    dref = np.zeros((B * n_src, C))
    np.add.at(dref, rows, gout.astype(np.float64))
    assert np.array_equal(out.detach().cpu().numpy(), x[rows])
    dx = xd.grad.cpu().double().numpy()
    assert_close(dx, dref, 1e-6, 'gather grad')
    unused = np.setdiff1d(np.arange(B * n_src), rows)
    assert unused.size > 0 and np.all(dx[unused] == 0.0)
    if form == 'hub':
        assert_close(dx[17], dref[17], 1e-6, 'hub row')


# ------------------------------------------------------------------ 4. the affine form
@pytest.mark.parametrize('form,K,C', [('dense', 16, 8), ('dense', 5, 132), ('padded', 5, 132), ('padded', 16, 8)])
def test_maxpool_affine_forward_and_its_backward(form, K, C):
    """crfconv_neighbor_maxpool_affine_forward called as _MLPBlockPool.forward calls it: out = max_k fmaf(a, x, b) with a of both
    signs (a < 0: the max is a min of x) and exactly 0 (every candidate ties: the first valid column wins).  Values to 1e-6 of float64
    (one fp32 rounding); arg equals the float64 argmax column wherever the float64 top two are further apart than rounding; that arg
    fed to crfconv_neighbor_maxpool_backward gives the float64 scatter."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    rng = np.random.default_rng(K * 1000 + C + (7 if form == 'padded' else 0))
    if form == 'dense':
        tab, _ = dense_table(rng, 2, 77, 300, K)
    else:
        tab, _, _, deg = edge_table(rng, 257, 190, (0, 1, 2, 5) if K == 5 else (0, 1, 2, 5, 16))
    rows = device_rows(tab)
    m_tgt, m_src = tab.m_tgt, tab.m_src
    assert tab.K == K and rows.shape == (m_tgt, K)
    x = rng.standard_normal((m_src, C)).astype(np.float32)
    a = rng.standard_normal(C).astype(np.float32)
    a[0::4] = 0.0
    a[1], a[2] = -abs(a[1]) - 0.5, abs(a[2]) + 0.5
    b = rng.standard_normal(C).astype(np.float32)
    assert (a > 0).any() and (a < 0).any() and (a == 0).any()
    coef = np.concatenate([a, b, rng.standard_normal(2 * C).astype(np.float32)])      # [a | b | two rows the pool does not read]
    gout = rng.standard_normal((m_tgt, C)).astype(np.float32)
    x64, a64, b64 = x.astype(np.float64), a.astype(np.float64), b.astype(np.float64)
    skip = near_tie_mask(x64, rows, a64, b64)
    skip[:, a == 0] = False                                             # exact ties by construction: the first-valid rule is checked there
    assert skip.mean() < 0.1                                            # mostly rows that name their best source twice
    gout[skip] = 0.0
    ref, rarg, dref = ref_pool(x64, rows, gout.astype(np.float64), a64, b64)
    first_valid = np.where((rows >= 0).any(1), 0, -1)                    # real entries lead in both table forms
    assert np.all(rarg[:, a == 0] == first_valid[:, None])

    xd, cd, gd = t(x), t(coef), t(gout)
    out = torch.empty((m_tgt, C), dtype=torch.float32, device=DEV)
    arg = torch.empty((m_tgt, C), dtype=torch.int32, device=DEV)
    _lib.call('crfconv_neighbor_maxpool_affine_forward', ptr(xd), ptr(cd), ptr(tab.idx32), tab.K, m_tgt, C, ptr(out), ptr(arg), stream_ptr())
    assert_close(out, ref, 1e-6, 'affine out')
    got = arg.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[:, a == 0], rarg[:, a == 0])               # a == 0: the first valid column (-1: no valid column)
    assert np.array_equal(got[~skip], rarg[~skip])
    if form == 'padded':
        empty = deg == 0
        assert np.array_equal(out.cpu().numpy()[empty], np.zeros((empty.sum(), C), dtype=np.float32)) and np.all(got[empty] == -1)

    rev_ptr, rev_eid = tab.reverse
    poison((m_src, C))
    dx = torch.empty((m_src, C), dtype=torch.float32, device=DEV)
    _lib.call('crfconv_neighbor_maxpool_backward', ptr(gd), ptr(arg), ptr(rev_ptr), ptr(rev_eid), tab.K, m_src, C, ptr(dx), stream_ptr())
    assert_close(dx, dref, 1e-6, 'affine grad')


# ------------------------------------------------------------------ 5. the fused node
def pool_block_case(K, Ci, Co, seed):
    """Inputs of one mlp_block_pool case and its float64 reference, all on the CPU: Linear -> BatchNorm1d (train) -> gather -> max
    over a table WITHOUT a doubled source in a row (two columns of one source tie exactly and lead to the same row: no near-tie in the
    sense below).  The upstream gradient is zero where the float64 top two are within rounding of each other."""
    m_src, n_tgt = 4100, 1025
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(m_src, generator=g)[:K] for _ in range(n_tgt)]).unsqueeze(0)
    x = torch.randn(m_src, Ci, generator=g) + 0.5
    W = torch.randn(Co, Ci, generator=g) / np.sqrt(Ci)
    gamma = (torch.rand(Co, generator=g) + 0.5) * torch.where(torch.arange(Co) % 3 == 1, -1.0, 1.0)      # mixed sign
    beta = torch.rand(Co, generator=g) * 0.6 - 0.3
    go = torch.randn(n_tgt, Co, generator=g)
    g2 = torch.randn(m_src, Ci, generator=g)                            # gradient of the fork's other consumer
    return dict(idx=idx, x=x, W=W, gamma=gamma, beta=beta, go=go, g2=g2)


def pool_block_reference(case, rows, fork):
    """float64 reference over the DEVICE's column order `rows`; returns the tensors to compare, the near-tie mask and its share."""
    Co = case['W'].shape[0]
    ref = torch.nn.BatchNorm1d(Co).double().train()
    with torch.no_grad():
        ref.weight.copy_(case['gamma'].double()); ref.bias.copy_(case['beta'].double())
    xr = case['x'].double().requires_grad_(True)
    Wr = case['W'].double().requires_grad_(True)
    z = ref(xr @ Wr.t())
    mask = near_tie_mask(z.detach().numpy(), rows)
    go = case['go'].clone()
    go[torch.from_numpy(mask)] = 0.0
    pooled = z[torch.from_numpy(rows)].max(1)[0]
    loss = (pooled * go.double()).sum()
    if fork:
        loss = loss + (xr * case['g2'].double()).sum()
    loss.backward()
    return dict(out=pooled.detach(), dx=xr.grad, dW=Wr.grad, dgamma=ref.weight.grad, dbeta=ref.bias.grad,
                running_mean=ref.running_mean, running_var=ref.running_var), go, float(mask.mean())


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('K,Ci,Co,fork', [(16, 32, 64, False), (5, 64, 128, False), (5, 32, 64, False), (16, 64, 128, False),
                                          (16, 32, 64, True)])
def test_mlp_block_pool_fused_node(K, Ci, Co, fork):
    """ops.mlp_block_pool (_MLPBlockPool: MFMA Linear with statistic records -> BatchNorm coefficients -> affine pool, and the fused
    backward) against float64 torch with autograd; gammas of mixed sign.  fork: the alias's gradient is added inside the node's
    backward -- the reference feeds x to both consumers.  Bounds as test_mlp_block_fused_backward states them for the same tensors.
    Masked share of the (target, channel) entries, from the float64 reference (cap 1 %): 0, 7.6e-6, 1.5e-5, 1.5e-5, 0 for the five
    cases in the order of the list.  Largest errors measured on the MI355X over the five cases (tol_baseline.json holds each):
    out 4.0e-7, dx 4.6e-7, dW 1.4e-7, dgamma 2.3e-7, dbeta 7.0e-8, running_mean 8.1e-9, running_var 5.9e-8."""
    from crfconv_amd import ops
    from crfconv_amd.graph import NeighborTable
    case = pool_block_case(K, Ci, Co, seed=K + Ci + Co)
    tab = NeighborTable(t(case['idx'].numpy()), 4100)
    rows = device_rows(tab)
    assert all(len(np.unique(r)) == K for r in rows[:64])
    ref, go, share = pool_block_reference(case, rows, fork)
    print('mlp_block_pool K=%d Ci=%d Co=%d fork=%s: masked share %.3e of the entries (cap 1e-2)' % (K, Ci, Co, fork, share))
    assert share <= 0.01

    x = case['x'].to(DEV).requires_grad_(True)
    W = case['W'].to(DEV).requires_grad_(True)
    bn = torch.nn.BatchNorm1d(Co)
    with torch.no_grad():
        bn.weight.copy_(case['gamma']); bn.bias.copy_(case['beta'])
    bn = bn.to(DEV).train()
    xin = x * 1.0 if fork else x                                         # fork: a non-leaf input, as inside the network
    res = ops.mlp_block_pool(xin, W, bn, tab, fork=fork)
    assert res is not None                                               # the fused path ran
    if fork:
        out, alias = res
        assert '_MLPBlockPool' in out.grad_fn.name() and '_MLPBlockPool' in alias.grad_fn.name()
        loss = (out * go.to(DEV)).sum() + (alias * case['g2'].to(DEV)).sum()
    else:
        out = res
        assert '_MLPBlockPool' in out.grad_fn.name()
        loss = (out * go.to(DEV)).sum()
    loss.backward()
    assert_close(out, ref['out'], 1e-5, 'out')
    assert_close(x.grad, ref['dx'], 2e-5, 'dx')
    assert_close(W.grad, ref['dW'], 2e-5, 'dW')
    assert_close(bn.weight.grad, ref['dgamma'], 2e-5, 'dgamma')
    assert_close(bn.bias.grad, ref['dbeta'], 2e-5, 'dbeta')
    assert_close(bn.running_mean, ref['running_mean'], 1e-6, 'running_mean')
    assert_close(bn.running_var, ref['running_var'], 1e-5, 'running_var')
    assert int(bn.num_batches_tracked) == 1


# ------------------------------------------------------------------ 6. residual join and LeakyReLU
def join_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a, b, go = (torch.randn(shape, generator=g) for _ in range(3))
    n = a.numel()
    pick = torch.randperm(n, generator=g)[:max(1, n // 10)]
    b.view(-1)[pick] = -a.view(-1)[pick]                                 # a + b == 0 exactly: forward 0, backward the `slope` branch
    return a, b, go, pick


@pytest.mark.parametrize('slope', [0.1, 1.0])
@pytest.mark.parametrize('shape', [(1,), (3,), (4,), (5,), (1023,), (1025,), (7, 9), (2, 3, 5)], ids=lambda s: 'x'.join(map(str, s)))
def test_add_lrelu_any_element_count(shape, slope):
    """ops.add_lrelu: one fp32 add and one multiply per element, forward and backward -- equal to torch's fp32 leaky_relu(a + b) and
    its autograd bit for bit, also through the padding of element counts that are no multiple of 4; both addends get the same gradient."""
    from crfconv_amd import ops
    a, b, go, pick = join_inputs(shape, sum(shape))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.leaky_relu(ar + br, slope)
    ref.backward(go)
    assert bool((ref.detach().view(-1)[pick] == 0).all())
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = ops.add_lrelu(ad, bd, slope)
    assert out.shape == ref.shape
    out.backward(go.to(DEV))
    assert torch.equal(out.detach().cpu(), ref.detach())
    assert torch.equal(ad.grad.cpu(), ar.grad)
    assert torch.equal(bd.grad, ad.grad)
    assert torch.equal(ad.grad.cpu().view(-1)[pick], (go * slope).view(-1)[pick])


@pytest.mark.parametrize('slope', [0.1, 1.0])
@pytest.mark.parametrize('shape', [(4,), (1024,), (257, 12)], ids=lambda s: 'x'.join(map(str, s)))
def test_leaky_relu_reuses_the_backward_kernel(shape, slope):
    """ops.leaky_relu (the join's backward kernel applied forward): exact against torch's fp32 leaky_relu and its autograd, zeros included."""
    from crfconv_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    x, go = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    x.view(-1)[::7] = 0.0
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.leaky_relu(xr, slope)
    ref.backward(go)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.leaky_relu(xd, slope)
    out.backward(go.to(DEV))
    assert torch.equal(out.detach().cpu(), ref.detach())
    assert torch.equal(xd.grad.cpu(), xr.grad)


def test_join_and_leaky_relu_refuse_what_they_do_not_take():
    from crfconv_amd import ops
    from crfconv_amd._lib import CrfConvError
    for n in (1, 3, 5, 1023):
        with pytest.raises(CrfConvError):
            ops.leaky_relu(torch.randn(n, device=DEV), 0.1)
    a = torch.randn(8, device=DEV)
    with pytest.raises(CrfConvError):
        ops.add_lrelu(a, torch.randn(4, device=DEV), 0.1)
    with pytest.raises(CrfConvError):
        ops.add_lrelu(a, torch.randn(2, 4, device=DEV), 0.1)
    with pytest.raises(CrfConvError):
        ops.add_lrelu(a, torch.randn(8, device=DEV).double(), 0.1)
    with pytest.raises(CrfConvError):
        ops.add_lrelu(a.half(), a.half(), 0.1)
