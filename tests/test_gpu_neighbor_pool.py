"""-m gpu: ops.neighbor_pool -- scatter(x[j], i, dim=0, reduce='sum' | 'mean' | 'max' | 'min') over a NeighborTable (csrc/pool.hip:
crfconv_neighbor_pool_forward / _backward) -- and the reference's pooling helpers built on it (models/common.py: fps_pooling,
fps_max_pooling), against float64 numpy references driven by the table AS THE DEVICE HOLDS IT (tab.idx32 read back).  No entry is masked
out of any comparison.

Bounds, per element, with u = 2^-24, n the target row's degree and R the length of the source's reverse row (first-order bounds of a
sequential float32 sum, plus one rounding for a division; the 64-edge float partial sums added in double are no worse):

    sum forward         n u sum_k |x|                      sum backward        R u sum |g|
    mean forward        (n + 1) u sum_k |x| / n            mean backward       (R + 1) u sum |g / deg|
    max / min forward   exact                              max / min backward  R_w u sum |g| over the winning edges"""
import numpy as np
import pytest
import torch

from gpu_util import DEV, t

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
REDUCES = ('sum', 'mean', 'max', 'min')


# ------------------------------------------------------------------ references and helpers
def device_rows(tab):
    """The table as the kernels read it: int64 [m_tgt, K] GLOBAL source rows, -1 = no neighbour."""
    return tab.idx32.cpu().numpy().astype(np.int64)


def ref_pool(x64, rows, reduce, gout64):
    """float64 (out, dx, forward bound, backward bound) of `reduce` over the valid columns of `rows`; for max and min the FIRST valid
    column that attains the extreme wins and takes the whole gradient.  A row without a valid column gives 0 and sends no gradient."""
    m_src, C = x64.shape
    K = rows.shape[1]
    valid = rows >= 0
    deg = valid.sum(1)
    safe = np.where(valid, rows, 0)
    v = x64[safe]                                                       # [m_tgt, K, C]
    absx = (np.abs(v) * valid[:, :, None]).sum(1)
    dx, absg = np.zeros_like(x64), np.zeros_like(x64)
    if reduce in ('sum', 'mean'):
        out = (v * valid[:, :, None]).sum(1)
        div = np.maximum(deg, 1)[:, None].astype(np.float64)
        if reduce == 'mean':
            out, fb = out / div, (deg[:, None] + 1) * U * absx / div
            w = gout64 / div
        else:
            fb, w = deg[:, None] * U * absx, gout64
        per_edge = np.broadcast_to(w[:, None, :], (rows.shape[0], K, C))[valid]
        np.add.at(dx, rows[valid], per_edge)
        np.add.at(absg, rows[valid], np.abs(per_edge))
        R = np.bincount(rows[valid], minlength=m_src)[:, None] + (1 if reduce == 'mean' else 0)
        return out, dx, fb, R * U * absg
    sign = 1.0 if reduce == 'max' else -1.0
    vv = np.where(valid[:, :, None], sign * v, -np.inf)
    arg = vv.argmax(1)                                                  # numpy's argmax: the first column at the maximum
    out = sign * np.take_along_axis(vv, arg[:, None, :], 1)[:, 0, :]
    out[deg == 0] = 0.0
    sel = np.broadcast_to((deg > 0)[:, None], arg.shape)
    src = np.take_along_axis(safe, arg, 1)                              # [m_tgt, C] winning source row
    cols = np.broadcast_to(np.arange(C), arg.shape)
    Rw = np.zeros_like(x64)
    np.add.at(dx, (src[sel], cols[sel]), gout64[sel])
    np.add.at(absg, (src[sel], cols[sel]), np.abs(gout64[sel]))
    np.add.at(Rw, (src[sel], cols[sel]), 1.0)
    return out, dx, np.zeros_like(out), Rw * U * absg


def poison(shape):
    """A freed device block of this shape full of NaN: the torch.empty the backward allocates next tends to reuse it, so a gradient
    row that the kernel leaves unwritten shows as NaN, not as a zero that happened to lie there."""
    torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()


def run_pool(x, tab, reduce, gout, op=None):
    """ops.neighbor_pool forward + backward (after a NaN-poisoned allocation) on float32 host arrays -> (out, dx) float32 tensors on
    the host."""
    from crfconv_amd import ops
    xd = t(x).requires_grad_(True)
    out = ops.neighbor_pool(xd, tab, reduce) if op is None else op(xd)
    assert out.shape == (tab.m_tgt, x.shape[1]) and out.dtype == torch.float32
    poison(tuple(xd.shape))
    out.backward(t(gout))
    return out.detach().cpu(), xd.grad.cpu()


def within(got, ref, bound, what):
    """|got - ref| <= bound element by element (float64); the largest error and the largest error / bound are printed first."""
    got = got.double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err > 0, err / bound, 0.0)
    print('[within] %-28s max err %.3e  max err / bound %.3f' % (what, err.max(), ratio.max()), flush=True)
    assert (err <= bound).all(), '%s: %d entries beyond their bound, worst err / bound %.3f' % (what, int((err > bound).sum()), ratio.max())


def check(x, tab, reduce, gout, what):
    """One forward + backward of `reduce` against the float64 reference with the bounds of the module's table -> (out, dx)."""
    rows = device_rows(tab)
    ref, dref, fb, bb = ref_pool(x.astype(np.float64), rows, reduce, gout.astype(np.float64))
    out, dx = run_pool(x, tab, reduce, gout)
    if reduce in ('max', 'min'):
        assert np.array_equal(out.double().numpy(), ref), '%s %s forward is not exact' % (what, reduce)
    else:
        within(out, ref, fb, '%s %s forward' % (what, reduce))
    within(dx, dref, bb, '%s %s backward' % (what, reduce))
    return out, dx


def dense_table(rng, B, n_tgt, n_src, K):
    from crfconv_amd.graph import NeighborTable
    return NeighborTable(t(rng.integers(0, n_src, (B, n_tgt, K))), n_src)


def padded_table(rng, n_tgt, n_src):
    """A padded table from a shuffled edge list with in-degrees from {0, 1, 2, 5} (each occurs), the last target empty, target 4 naming
    one source twice, and the upper quarter of the sources named by no edge."""
    from crfconv_amd.graph import table_from_edges
    deg = rng.choice(np.asarray((0, 1, 2, 5)), n_tgt)
    deg[:5] = (0, 1, 2, 5, 2)
    deg[-1] = 0
    tgt = np.repeat(np.arange(n_tgt), deg)
    src = rng.integers(0, n_src - n_src // 4, tgt.size)
    src[tgt == 4] = 11
    perm = rng.permutation(tgt.size)
    tgt, src = tgt[perm], src[perm]
    tab = table_from_edges(t(tgt), t(src), n_tgt, n_src)
    assert tab.padded and tab.K == 5 and tab.n_edges == tgt.size
    return tab, tgt, src, deg


# ------------------------------------------------------------------ 1. dense tables
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('K,C', [(1, 4), (3, 8), (4, 36), (5, 132), (7, 8), (16, 4), (33, 36), (64, 8), (5, 6)])
def test_pool_dense_table_shapes(K, C, reduce):
    """K % 4 != 0 takes the tail guard of the four-neighbour trip, a K that is no power of two the integer divide of the backward's
    edge id -> target row, K = 1 the instantiation without that divide; C = 6 goes through the channel-padding wrapper."""
    B, n_src, n_tgt = 2, 300, 77
    rng = np.random.default_rng(1000 * K + C)
    tab = dense_table(rng, B, n_tgt, n_src, K)
    rows = device_rows(tab)
    assert rows.shape == (B * n_tgt, K) and rows.min() >= 0 and not tab.padded
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    _, dx = check(x, tab, reduce, gout, 'dense K=%d C=%d' % (K, C))
    unused = np.setdiff1d(np.arange(B * n_src), rows)                   # (none left at the widest tables)
    assert bool((dx[unused] == 0.0).all())


# ------------------------------------------------------------------ 2. padded tables
@pytest.mark.parametrize('C', [4, 36])
def test_pool_padded_table(C):
    """-1 slots are skipped: an empty target is exactly 0 for every reduction and sends no gradient, the mean divides by the real
    degree, a source without a reverse edge gets an exact zero gradient row, and a row naming one source twice counts it twice in sum and
    mean.  The same entries as a table_from_index table give the same bits."""
    from crfconv_amd import ops
    from crfconv_amd.graph import table_from_index
    n_tgt, n_src = 257, 190
    rng = np.random.default_rng(257 + C)
    tab, tgt, src, deg = padded_table(rng, n_tgt, n_src)
    rows = device_rows(tab)
    assert np.array_equal((rows >= 0).sum(1), deg) and (deg == 0).sum() > 10 and rows[4].tolist() == [11, 11, -1, -1, -1]
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    no_edge = np.setdiff1d(np.arange(n_src), src)
    assert no_edge.size >= n_src // 4
    one = np.nonzero(deg == 1)[0]
    tab2 = table_from_index(tab.idx32.clone(), n_src)
    for reduce in REDUCES:
        out, dx = check(x, tab, reduce, gout, 'padded C=%d' % C)
        assert bool((out[deg == 0] == 0.0).all())
        assert bool((dx[no_edge] == 0.0).all())
        assert torch.equal(out[one], torch.from_numpy(x[rows[one, 0]]))           # degree 1: the row itself, the mean divides by 1
        twice = torch.from_numpy(x[11])
        assert torch.equal(out[4], twice + twice if reduce == 'sum' else twice)  # (x + x) / 2 is x exactly
        out2, dx2 = run_pool(x, tab2, reduce, gout)
        assert torch.equal(out2, out) and torch.equal(dx2, dx)
    # the duplicated source's gradient holds target 4's entry twice: with every other gradient row zero it is exactly 2 g (sum), g (mean)
    g4 = np.zeros_like(gout)
    g4[4] = gout[4]
    for reduce, f in (('sum', 2.0), ('mean', 1.0)):
        _, dx = run_pool(x, tab, reduce, g4)
        assert torch.equal(dx[11], torch.from_numpy(f * gout[4])) and int((dx != 0).any(1).sum()) == 1
    assert ops.neighbor_pool(t(x), tab, 'add').equal(ops.neighbor_pool(t(x), tab, 'sum'))


def test_pool_table_without_edges_and_without_rows():
    """E = 0 (one column of -1): every output and gradient is an exact zero.  m_tgt = 0: zeros without a library call."""
    from crfconv_amd import ops
    from crfconv_amd.graph import table_from_edges
    n_tgt, n_src, C = 257, 190, 8
    none = torch.empty(0, dtype=torch.long, device=DEV)
    tab = table_from_edges(none, none, n_tgt, n_src)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    empty = table_from_edges(none, none, 0, n_src)
    for reduce in REDUCES:
        out, dx = run_pool(x, tab, reduce, gout)
        assert bool((out == 0).all()) and bool((dx == 0).all())
        res = ops.neighbor_pool(t(x), empty, reduce)
        assert res.shape == (0, C) and res.dtype == torch.float32


# ------------------------------------------------------------------ 3. a heavy reverse row
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
def test_pool_heavy_reverse_row(reduce):
    """1031 targets, K = 3, every entry source 0 of 40: a reverse row of 3093 edges, summed 64 edges per float partial."""
    from crfconv_amd.graph import NeighborTable
    n_src, n_tgt, K, C = 40, 1031, 3, 8
    tab = NeighborTable(t(np.zeros((1, n_tgt, K), dtype=np.int64)), n_src)
    assert int(tab.idx32.abs().max()) == 0
    rng = np.random.default_rng(1031)
    x = rng.standard_normal((n_src, C)).astype(np.float32)
    gout = rng.standard_normal((n_tgt, C)).astype(np.float32)
    _, dx = check(x, tab, reduce, gout, 'hub')
    assert bool((dx[1:] == 0).all()) and bool((dx[0] != 0).all())


# ------------------------------------------------------------------ 4. identities against code this family does not touch
def entry_forward(x, tab, reduce, want_count=False):
    """crfconv_neighbor_pool_forward called directly -> (out, arg, count) on the host."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    xd = t(x)
    C = x.shape[1]
    out = torch.full((tab.m_tgt, C), float('nan'), dtype=torch.float32, device=DEV)
    arg = torch.full((tab.m_tgt, C), -7, dtype=torch.int32, device=DEV)
    count = torch.full((tab.m_tgt,), -7, dtype=torch.int32, device=DEV) if want_count else None
    _lib.call('crfconv_neighbor_pool_forward', ptr(xd), ptr(tab.idx32), tab.K, tab.m_tgt, C, reduce, ptr(out), ptr(arg), ptr(count),
              stream_ptr())
    return out.cpu(), arg.cpu(), None if count is None else count.cpu()


@pytest.mark.parametrize('form,K,C', [('dense', 16, 8), ('dense', 5, 132), ('padded', 5, 36)])
def test_pool_max_is_the_affine_kernel_with_unit_coefficients(form, K, C):
    """fmaf(1, x, 0) is x: out and arg of reduce = 2 equal crfconv_neighbor_maxpool_affine_forward(a = 1, b = 0) bit for bit; the min's
    arg is the max's of -x; sum and mean leave arg alone; count is the row's degree for every reduction."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    rng = np.random.default_rng(K * 100 + C)
    tab = dense_table(rng, 2, 77, 300, K) if form == 'dense' else padded_table(rng, 257, 190)[0]
    x = rng.standard_normal((tab.m_src, C)).astype(np.float32)
    x[::3] = np.round(x[::3])                                           # ties between different sources as well
    xd = t(x)
    coef = t(np.concatenate([np.ones(C), np.zeros(3 * C)]).astype(np.float32))
    ref = torch.empty((tab.m_tgt, C), dtype=torch.float32, device=DEV)
    rarg = torch.empty((tab.m_tgt, C), dtype=torch.int32, device=DEV)
    _lib.call('crfconv_neighbor_maxpool_affine_forward', ptr(xd), ptr(coef), ptr(tab.idx32), tab.K, tab.m_tgt, C, ptr(ref), ptr(rarg),
              stream_ptr())
    deg = torch.from_numpy((device_rows(tab) >= 0).sum(1).astype(np.int32))
    out, arg, count = entry_forward(x, tab, 2, want_count=True)
    assert torch.equal(out, ref.cpu()) and torch.equal(arg, rarg.cpu()) and torch.equal(count, deg)
    assert torch.equal(entry_forward(x, tab, 2)[0], out)
    mout, marg, mcount = entry_forward(-x, tab, 3, want_count=True)
    assert torch.equal(mout, -out) and torch.equal(marg, arg) and torch.equal(mcount, deg)
    for reduce in (0, 1):
        _, sarg, scount = entry_forward(x, tab, reduce, want_count=True)
        assert bool((sarg == -7).all()) and torch.equal(scount, deg)


@pytest.mark.parametrize('form,K,C', [('dense', 16, 8), ('dense', 7, 6), ('padded', 5, 36)])
def test_pool_max_and_min_against_neighbor_maxpool(form, K, C):
    """neighbor_pool(x, 'max') is ops.neighbor_maxpool, outputs and gradients; neighbor_pool(x, 'min') is -neighbor_pool(-x, 'max')."""
    from crfconv_amd import ops
    rng = np.random.default_rng(K * 100 + C + 1)
    tab = dense_table(rng, 2, 77, 300, K) if form == 'dense' else padded_table(rng, 257, 190)[0]
    x = rng.standard_normal((tab.m_src, C)).astype(np.float32)
    x[::3] = np.round(x[::3])
    gout = rng.standard_normal((tab.m_tgt, C)).astype(np.float32)
    out, dx = run_pool(x, tab, 'max', gout)
    old, dold = run_pool(x, tab, None, gout, op=lambda xd: ops.neighbor_maxpool(xd, tab))
    assert torch.equal(out, old) and torch.equal(dx, dold)
    mn, dmn = run_pool(x, tab, 'min', gout)
    neg, dneg = run_pool(x, tab, None, gout, op=lambda xd: -ops.neighbor_pool(-xd, tab, 'max'))
    assert torch.equal(mn, neg) and torch.equal(dmn, dneg)
    assert bool((mn <= out).all())


@pytest.mark.parametrize('C', [4, 132, 6])
def test_pool_sum_over_a_one_column_table_is_gather_rows(C):
    from crfconv_amd import ops
    from crfconv_amd.graph import NeighborTable
    B, n_src, n_tgt = 2, 300, 1031
    rng = np.random.default_rng(C)
    up = rng.integers(0, n_src, (B, n_tgt, 1))
    up[0] = 17                                                          # a reverse row of 1031 edges
    tab = NeighborTable(t(up), n_src)
    x = rng.standard_normal((B * n_src, C)).astype(np.float32)
    gout = rng.standard_normal((B * n_tgt, C)).astype(np.float32)
    ref, dref = run_pool(x, tab, None, gout, op=lambda xd: ops.gather_rows(xd, tab))
    for reduce in ('sum', 'mean'):                                      # (the mean of one row is the row: g / 1.0f is g)
        out, dx = run_pool(x, tab, reduce, gout)
        assert torch.equal(out, ref) and torch.equal(dx, dref)


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize('reduce', REDUCES)
def test_pool_is_deterministic(reduce):
    rng = np.random.default_rng(5)
    tab = dense_table(rng, 2, 1031, 300, 16)                            # reverse rows of ~55 edges on average, some beyond 64
    x = rng.standard_normal((600, 36)).astype(np.float32)
    gout = rng.standard_normal((2062, 36)).astype(np.float32)
    a = run_pool(x, tab, reduce, gout)
    b = run_pool(x, tab, reduce, gout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 6. fps_pooling / fps_max_pooling
def scatter_reference(x64, i, j, n_tgt, reduce):
    """float64 scatter(x[j], i, dim=0, reduce=) over an edge list -> (out, bound)."""
    C = x64.shape[1]
    n = np.bincount(i, minlength=n_tgt)[:, None].astype(np.float64)
    absx = np.zeros((n_tgt, C))
    np.add.at(absx, i, np.abs(x64[j]))
    if reduce == 'max':
        out = np.full((n_tgt, C), -np.inf)
        np.maximum.at(out, i, x64[j])
        out[n[:, 0] == 0] = 0.0
        return out, np.zeros_like(out)
    out = np.zeros((n_tgt, C))
    np.add.at(out, i, x64[j])
    if reduce == 'mean':
        return out / np.maximum(n, 1), (n + 1) * U * absx / np.maximum(n, 1)
    return out, n * U * absx


@pytest.fixture(scope='module', params=[(200, 57), (9, 40), (9,)], ids=lambda s: '+'.join(map(str, s)))
def clouds(request):
    """Clouds of the given sizes: 200 + 57 is the case of the specification; 9 + 40 has rows of 9 neighbours padded to k = 16; 9 alone
    is one cloud without a batch vector."""
    sizes = request.param
    rng = np.random.default_rng(sum(sizes))
    N = sum(sizes)
    single = len(sizes) == 1
    return dict(sizes=sizes, pos=t(rng.random((N, 3)).astype(np.float32)), x=t(rng.standard_normal((N, 12)).astype(np.float32)),
                edge_attr=t(rng.standard_normal((N, 5)).astype(np.float32)),
                batch=None if single else t(np.repeat(np.arange(len(sizes)), sizes)),
                ptr=t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)))


@pytest.mark.parametrize('reduce', ['sum', 'mean', 'max'])
def test_fps_pooling(clouds, reduce):
    from crfconv_amd.models import common, graph_ops
    pos, x, ea, batch, ptr, sizes = (clouds[k] for k in ('pos', 'x', 'edge_attr', 'batch', 'ptr', 'sizes'))
    k, r = 16, 0.25
    idx = graph_ops.fps(pos, batch, r)
    picks = [int(np.ceil(r * n)) for n in sizes]
    assert idx.numel() == sum(picks)
    sub = None if batch is None else batch[idx]
    edges = graph_ops.knn(pos, pos[idx], k, batch, sub).cpu().numpy()
    assert edges.shape[1] == sum(p * min(k, n) for p, n in zip(picks, sizes))
    ref, bound = scatter_reference(x.cpu().double().numpy(), edges[0], edges[1], idx.numel(), reduce)

    px, ppos, pea, pbatch = common.fps_pooling(pos, x, ea, batch, k, r, reduce)
    if reduce == 'max':
        assert np.array_equal(px.cpu().double().numpy(), ref)
    else:
        within(px.cpu(), ref, bound, 'fps_pooling %s' % reduce)
    assert torch.equal(ppos, pos[idx]) and torch.equal(pea, ea[idx])
    assert pbatch is None if batch is None else torch.equal(pbatch, batch[idx])

    qx, qpos, qea, qptr = common.fps_pooling(pos, x, ea, k=k, r=r, reduce=reduce, ptr=ptr)
    assert torch.equal(qx, px) and torch.equal(qpos, ppos) and torch.equal(qea, pea)
    assert qptr.dtype == torch.int64 and qptr.tolist() == np.concatenate([[0], np.cumsum(picks)]).tolist()
    if reduce == 'max':
        mx, mpos, mbatch = common.fps_max_pooling(pos, x, batch, k, r)
        assert torch.equal(mx, px) and torch.equal(mpos, ppos)
        assert mbatch is None if batch is None else torch.equal(mbatch, pbatch)
        mx, mpos, mptr = common.fps_max_pooling(pos, x, k=k, r=r, ptr=ptr)
        assert torch.equal(mx, px) and torch.equal(mpos, ppos) and torch.equal(mptr, qptr)
    if reduce == 'sum':
        assert torch.equal(common.fps_pooling(pos, x, ea, batch, k, r, 'add')[0], px)


def test_fps_pooling_sends_gradients_through_the_table():
    """The sum's gradient through fps_pooling: every point gets the sum of the gradients of the picks whose k nearest hold it."""
    from crfconv_amd.models import common, graph_ops
    rng = np.random.default_rng(77)
    sizes = (200, 57)
    pos = t(rng.random((257, 3)).astype(np.float32))
    batch = t(np.repeat(np.arange(2), sizes))
    x = t(rng.standard_normal((257, 12)).astype(np.float32)).requires_grad_(True)
    ea = t(rng.standard_normal((257, 5)).astype(np.float32))
    px = common.fps_pooling(pos, x, ea, batch, 16, 0.25, 'sum')[0]
    assert '_NeighborPool' in px.grad_fn.name()                         # one autograd node (C = 12: no channel padding)
    g = rng.standard_normal(tuple(px.shape)).astype(np.float32)
    px.backward(t(g))
    idx = graph_ops.fps(pos, batch, 0.25)
    e = graph_ops.knn(pos, pos[idx], 16, batch, batch[idx]).cpu().numpy()
    dref, absg = np.zeros((257, 12)), np.zeros((257, 12))
    np.add.at(dref, e[1], g.astype(np.float64)[e[0]])
    np.add.at(absg, e[1], np.abs(g.astype(np.float64))[e[0]])
    within(x.grad.cpu(), dref, np.bincount(e[1], minlength=257)[:, None] * U * absg, 'fps_pooling sum backward')
