"""-m gpu: the three operators of the label-space (discrete) CRF layer, one by one -- ops.kernel_weights (csrc/discrete.hip: forward,
target-side and source-side backward, each in the HPL = 1 / 2 / 4 form), ops.weighted_step (crfconv_meanfield_step, _bwd_edge,
_bwd_scatter with GIVEN weights) and ops.discrete_meanfield -- against float64 references written here in plain torch with autograd on
the CPU.  Every reference is driven by the table AS THE DEVICE HOLDS IT (tab.idx32 read back); tables come from table_from_index (holes
anywhere), NeighborTable (dense, columns 1.. re-sorted by the device) and table_from_edges (a shuffled edge list).

The comparison (`own_scale`) is gpu_util's anchored rule on each tensor's OWN scale: e = max|got - ref64| / max|ref64| may reach the bound
stated at the call, or 4 x the error e32 of the same reference run in float32, whichever is larger -- and e32 <= bound is asserted too, so
the second branch never decides a case (inputs are scaled for that: features in 0.05 .. 0.15 keep the kernel distances below ~1 and the
weights of order 0.1 .. 1).  Bounds are ~10 x the largest e32 a site measured on the CPU (another summation order); the largest e measured
on the MI355X stands beside each, in the test's docstring.  Sites that say "exact" compare with torch.equal.  Before each backward a NaN-filled block of every
gradient's shape is freed (`poison`), so a row a kernel leaves unwritten shows as NaN; every output is asserted finite."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, grad_errors, t

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def device_rows(tab):
    """The table as the kernels read it: int64 [m, K] source rows, -1 = no neighbour."""
    return tab.idx32.cpu().long()


def poison(*shapes):
    """Freed device blocks of these shapes full of NaN: the torch.empty calls of the next launch sequence tend to reuse them."""
    blocks = [torch.full(tuple(s), float('nan'), dtype=torch.float32, device=DEV) for s in shapes]
    torch.cuda.synchronize()
    del blocks


def errors(got, ref32, ref64):
    """(e, e32): max|got - ref64| and max|ref32 - ref64| over max|ref64| (gpu_util.grad_errors on one tensor, no floor: an all-zero
    reference makes any difference infinitely large)."""
    (_, e, e32, _, _), = grad_errors({'x': got}, {'x': ref32}, {'x': ref64}, floor=0.0)
    return e, e32


def own_scale(got, ref32, ref64, bound, what):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), '%s: shape %s, reference %s' % (what, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), '%s is not finite' % what
    e, e32 = errors(got, ref32, ref64)
    print('[own_scale] %-10s e %.3e  e32 %.3e  bound %.1e' % (what, e, e32, bound), flush=True)
    assert e32 <= bound, '%s: the float32 restatement itself misses the bound (%.3e > %.1e): rescale the inputs' % (what, e32, bound)
    assert e <= max(bound, 4.0 * e32), '%s: err vs fp64 on its own scale %.3e > max(%.1e, 4 x fp32 restatement %.3e)' % (what, e, bound, e32)
    return e, e32


def rejected(bent, ref32, ref64, bound):
    """True when own_scale's rule refuses `bent` (arithmetic on results already computed, no launch)."""
    e, e32 = errors(bent, ref32, ref64)
    return not e <= max(bound, 4.0 * e32)


def f32(rng, shape, lo, hi):
    return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32))


def leaf(v, dtype):
    """A fresh leaf of this dtype (a copy also where the dtype is the tensor's own)."""
    return v.detach().to(dtype).clone().requires_grad_(True)


def dev(v):
    """A float tensor's values in a fresh device tensor."""
    return v.detach().to(DEV).clone()


def index_table(rows):
    """int [m, K] source rows with -1 holes anywhere -> a padded table over the same m rows (graph.table_from_index)."""
    from crfconv_amd.graph import table_from_index
    rows = np.asarray(rows)
    return table_from_index(t(np.ascontiguousarray(rows.astype(np.int32))), rows.shape[0])


def dense_table(rows):
    """[m, K] without holes -> NeighborTable of one cloud (the device re-sorts columns 1..)."""
    from crfconv_amd.graph import NeighborTable
    rows = np.asarray(rows)
    assert rows.min() >= 0
    return NeighborTable(t(rows[None].astype(np.int64)), rows.shape[0])


def edges_table(rng, m, degrees):
    """table_from_edges from a SHUFFLED edge list whose in-degrees are drawn from `degrees` (each occurs; the last row has none)."""
    from crfconv_amd.graph import table_from_edges
    deg = rng.choice(np.asarray(degrees), m)
    deg[:len(degrees)] = degrees
    deg[-1] = 0
    tgt = np.repeat(np.arange(m), deg)
    src = rng.integers(0, m, tgt.size)
    perm = rng.permutation(tgt.size)
    tab = table_from_edges(t(tgt[perm]), t(src[perm]), m, m)
    assert tab.padded and tab.K == max(degrees) and tab.n_edges == tgt.size
    return tab


def shaped_rows(kind, rng, m, K):
    """[m, K] tables that each reach one branch of the kernels (the tests assert the property they are named for)."""
    rows = rng.integers(0, m, (m, K))
    holes = rng.random((m, K)) < 0.35
    hub = (min(5, m - 1), m - 1)
    if kind == 'hub':                                 # two sources every row points at; most rows have no in-edge
        rows = rng.integers(0, min(m, 40), (m, K))
        rows[:, K // 4], rows[:, K - 1] = hub
    elif kind == 'dup':                               # the same source twice in one row (every row), in every column (row 3)
        rows[:, K - 1] = rows[:, 0]
        rows[min(3, m - 1), :] = rows[min(3, m - 1), 0]
    elif kind == 'self':                              # self-loops in an interior column, in two columns of every 7th row
        rows[:, K // 2] = np.arange(m)
        rows[::7, 0] = np.arange(m)[::7]
    elif kind == 'holes':                             # -1 in interior and leading columns
        rows[holes] = -1
        rows[0, 0], rows[0, K - 1] = -1, 2 % m
    elif kind == 'empty':                             # rows without a valid entry: the first, one inside, the last
        rows[holes] = -1
        rows[[0, m // 2, m - 1]] = -1
    elif kind == 'none':                              # no edge at all
        rows[:] = -1
    else:                                             # 'ragged': all of it in one table
        assert kind == 'ragged'
        rows[:, K // 4], rows[:, K - 1] = hub
        rows[:, 1] = rows[:, 0]
        rows[::7, K // 2] = np.arange(m)[::7]
        rows[holes] = -1
        rows[[0, m // 2, m - 1]] = -1
    return rows


# ------------------------------------------------------------------ float64 / float32 references (plain torch, autograd)
def ref_kernel_weights(fk, Wg, rows, G, H, fk_src=None):
    """w[i, k] = sum_g Wg[g] exp(-|fk[j, g, :] - fk[i, g, :]|^2) for rows[i, k] = j >= 0, 0 elsewhere.  fk_src: a second leaf with fk's
    values read on the SOURCE side (row j): its gradient is the reverse-walk term of dfk alone.  Kernel by kernel and in row chunks: no
    intermediate above 2e7 elements."""
    m, K = rows.shape
    ft = fk.reshape(-1, G, H)
    fs = ft if fk_src is None else fk_src.reshape(-1, G, H)
    j = rows.clamp(min=0)
    step = max(1, int(2e7 // (K * H)))
    out = []
    for lo in range(0, m, step):
        jj = j[lo:lo + step]
        w = torch.zeros(jj.shape, dtype=fk.dtype)
        for g in range(G):
            d = ((fs[:, g][jj] - ft[lo:lo + step, g][:, None, :]) ** 2).sum(-1)
            w = w + Wg[g] * torch.exp(-d)
        out.append(w)
    return torch.where(rows >= 0, torch.cat(out), torch.zeros((), dtype=fk.dtype))


def ref_weighted_step(x, z, w, Q, P, rows):
    """z Q + (sum_k w_ik x_j) P over the valid entries."""
    valid = rows >= 0
    msg = (torch.where(valid, w, torch.zeros((), dtype=w.dtype))[:, :, None] * x[rows.clamp(min=0)]).sum(1)
    return z @ Q + msg @ P


def ref_discrete_meanfield(p, w, C, rows, steps):
    """oracle/crf_oracle.py discrete_crf, the loop: u = -log p, q_0 = p, q <- softmax(-u - (sum_e w_e q_j) C) over the table's valid entries."""
    valid = rows >= 0
    j = rows.clamp(min=0)
    wv = torch.where(valid, w, torch.zeros((), dtype=w.dtype))
    u = -torch.log(p)
    q = p
    for _ in range(steps):
        msg = (wv[:, :, None] * q[j]).sum(1)
        q = torch.softmax(-u - msg @ C, dim=-1)
    return q


def kw_reference(fk, Wg, rows, G, H, gw, dtype):
    """{w, dfk, dW, dfk_src}: dfk_src is the source-side (reverse-walk) part of dfk."""
    ft, fs, Wr = leaf(fk, dtype), leaf(fk, dtype), leaf(Wg, dtype)
    w = ref_kernel_weights(ft, Wr, rows, G, H, fk_src=fs)
    (w * gw.to(dtype)).sum().backward()
    return dict(w=w.detach(), dfk=ft.grad + fs.grad, dW=Wr.grad, dfk_src=fs.grad)


def kw_run(fk, Wg, tab, G, H, gw, fk_grad=True, W_grad=True):
    """ops.kernel_weights forward + backward on float32 host tensors (as given: a non-contiguous fk / gw goes in as it is)."""
    from crfconv_amd import ops
    fd = dev(fk).requires_grad_(fk_grad)
    Wd = dev(Wg).requires_grad_(W_grad)
    poison((fk.shape[0], tab.K))
    w = ops.kernel_weights(fd, Wd, tab, G, H)
    assert w.shape == (fk.shape[0], tab.K)
    poison(fk.shape, fk.shape, (fk.shape[0], tab.K))
    w.backward(dev(gw))
    assert (fd.grad is not None) == fk_grad and (Wd.grad is not None) == W_grad
    return dict(w=w.detach().cpu(), dfk=None if fd.grad is None else fd.grad.cpu(), dW=None if Wd.grad is None else Wd.grad.cpu())


def kw_inputs(rng, m, K, G, H):
    """Features in 0.05 .. 0.15 (distances below ~1 up to H = 256), kernel weights of either sign away from 0, a gradient of either sign whose mean is not 0
    (dW[g] is ONE sum over every edge: with a mean-zero gradient it cancels to ~1 / sqrt(edges) of its terms, and the float32 restatement,
    which sums in float32 where the kernel sums in float64, misses any bound near its own rounding)."""
    fk = f32(rng, (m, G * H), 0.05, 0.15)
    Wg = f32(rng, (G,), 0.2, 0.5) * torch.where(torch.arange(G) % 3 == 1, -0.3, 1.0)      # (the negative ones smaller: w does not cancel)
    gw = torch.from_numpy((1.0 + 0.5 * rng.standard_normal((m, K))).astype(np.float32))
    return fk, Wg, gw


def kw_check(fk, Wg, tab, G, H, gw, bounds):
    """One kernel_weights case: forward, dfk, dW within `bounds` = (w, dfk, dW) of float64 on their own scales; w exactly 0 on missing
    entries.  Returns (got, ref32, ref64, rows)."""
    rows = device_rows(tab)
    assert rows.shape == gw.shape and rows.shape[0] == fk.shape[0] and int(rows.max()) < fk.shape[0]
    r64 = kw_reference(fk, Wg, rows, G, H, gw, torch.float64)
    r32 = kw_reference(fk, Wg, rows, G, H, gw, torch.float32)
    got = kw_run(fk, Wg, tab, G, H, gw)
    for k, b in zip(('w', 'dfk', 'dW'), bounds):
        own_scale(got[k], r32[k], r64[k], b, k)
    assert bool((got['w'][rows < 0] == 0).all())
    return got, r32, r64, rows


# ------------------------------------------------------------------ (a) kernel_weights over widths and kernel counts
@pytest.mark.parametrize('G,H', [(3, 1), (3, 7), (3, 63), (3, 64), (3, 65), (3, 96), (3, 127), (3, 128), (3, 129), (3, 200), (3, 256),
                                 (1, 64), (2, 64), (7, 64), (8, 64), (1, 129), (2, 129), (7, 129), (8, 129)])
def test_kernel_weights_widths_and_kernel_counts(G, H):
    """Dense NeighborTable, m = 301 (one row in the last workgroup of 4), K = 9.  H = 1 .. 64: HPL = 1 (H = 1, 7, 63: a partly filled
    segment); 65 .. 128: HPL = 2 (65, 96, 127: partly filled second segment); 129 .. 256: HPL = 4 (129: one channel in the third segment,
    none in the fourth; 200: partly filled fourth); the seams 64 / 65 and 128 / 129 on both sides.  G = 1 and G = 8 (DW_GMAX) are the two
    ends of the `g < G` guards in the 8-way unrolled loops.
    Bounds: w 2e-6, dfk 2e-6, dW 2e-6 (float32 restatement on the CPU, largest of the 19 cases: 1.8e-7 / 1.8e-7 / 1.5e-7).
    Largest measured on the MI355X: w 1.7e-7, dfk 2.4e-7, dW 5.7e-8."""
    m, K = 301, 9
    rng = np.random.default_rng(1000 * G + H)
    tab = dense_table(rng.integers(0, m, (m, K)))
    assert not tab.padded
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    kw_check(fk, Wg, tab, G, H, gw, (2e-6, 2e-6, 2e-6))


# ------------------------------------------------------------------ (b) degrees
@pytest.mark.parametrize('K,G,H,m', [(1, 5, 64, 301), (2, 5, 64, 301), (16, 5, 64, 301), (33, 5, 64, 301), (64, 5, 64, 301), (64, 8, 256, 37)])
def test_kernel_weights_degrees(K, G, H, m):
    """K = 1 and K = 64 (the limit) and values between, on table_from_index tables with a few holes; K = 64 at the widest form
    (G = 8, H = 256: HPL = 4, every register of the unrolled loops live) on 37 rows.
    Bounds: w 2e-6, dfk 3e-6, dW 2e-6 (CPU float32 restatement, largest of the 6 cases: 1.7e-7 / 2.4e-7 / 9.9e-8).
    Largest measured on the MI355X: w 1.5e-7, dfk 5.2e-7, dW 5.9e-8."""
    rng = np.random.default_rng(100 * K + H)
    rows = rng.integers(0, m, (m, K))
    rows[rng.random((m, K)) < 0.05] = -1
    tab = index_table(rows)
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    kw_check(fk, Wg, tab, G, H, gw, (2e-6, 3e-6, 2e-6))


# ------------------------------------------------------------------ (c) row counts
@pytest.mark.parametrize('m', [1, 2, 3, 4, 5, 1237])
def test_kernel_weights_row_counts(m):
    """(K, G, H) = (8, 5, 32).  m < 4: one partly filled workgroup; 4: exactly one; 5: two float64 dW slabs, the second from one row;
    1237: 310 slabs, the last from one row.  m = 1: every entry is a self-loop, so dfk is exactly 0.
    Bounds: w 2e-6, dfk 2e-6, dW 2e-6 (CPU float32 restatement, largest of the 6 cases: 1.7e-7 / 1.3e-7 / 1.1e-7).
    Largest measured on the MI355X: w 1.4e-7, dfk 1.8e-7, dW 6.1e-8."""
    from crfconv_amd import _lib
    K, G, H = 8, 5, 32
    rng = np.random.default_rng(m)
    rows = rng.integers(0, m, (m, K))
    rows[:, 3][rng.random(m) < 0.3] = -1
    tab = index_table(rows)
    assert _lib.load().crfconv_kernel_weights_partials(m) == 8 * ((m + 3) // 4)
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    got, _, _, _ = kw_check(fk, Wg, tab, G, H, gw, (2e-6, 2e-6, 2e-6))
    if m == 1:
        assert torch.equal(got['dfk'], torch.zeros_like(got['dfk']))


# ------------------------------------------------------------------ (d) table shapes
@pytest.mark.parametrize('kind,G,H', [('hub', 5, 64), ('dup', 5, 64), ('self', 5, 64), ('holes', 5, 64), ('empty', 5, 64), ('none', 5, 64),
                                      ('edges', 5, 64), ('ragged', 2, 200)])
def test_kernel_weights_table_shapes(kind, G, H):
    """The reverse-CSR walk of kw_backward_source_kernel over uneven in-degrees and the `j < 0` branches of all three kernels; m = 301,
    K = 9 (edges: up to 12).  'ragged' has hub, duplicates, self-loops, holes and empty rows in one table at (G, H) = (2, 200), HPL = 4.
    hub: the comparison must be able to fail -- bent results (arithmetic on what was computed) are refused.
    Bounds: w 2e-6, dfk 6e-6, dW 2e-6 (CPU float32 restatement, largest of the 8 cases: 2.1e-7 / 6.3e-7 / 1.4e-7).
    Largest measured on the MI355X: w 1.6e-7, dfk 5.2e-7, dW 4.0e-8."""
    m, K = 301, 9
    rng = np.random.default_rng(sum(map(ord, kind)) + H)
    tab = edges_table(rng, m, tuple(range(13))) if kind == 'edges' else index_table(shaped_rows(kind, rng, m, K))
    rows = device_rows(tab)
    valid = rows >= 0
    indeg = torch.bincount(rows[valid], minlength=m)
    if kind in ('hub', 'ragged'):
        assert int(indeg[5]) >= (m if kind == 'hub' else m // 3) and int(indeg[m - 1]) >= (m if kind == 'hub' else m // 3)
    if kind == 'hub':
        assert int((indeg == 0).sum()) > m // 2                         # sources no row points at: dfk = dfk_self
    if kind in ('dup', 'ragged'):
        assert bool(((rows[:, 0] == rows[:, -1 if kind == 'dup' else 1]) & valid[:, 0]).any())
    if kind in ('self', 'ragged'):
        assert bool((rows == torch.arange(m)[:, None]).any())
    if kind in ('holes', 'ragged'):
        assert bool((~valid[:, :-1] & valid[:, 1:]).any())                # a hole in front of a valid entry
    if kind in ('empty', 'ragged', 'edges'):
        assert not valid[m - 1].any() and int((~valid.any(1)).sum()) >= 2 and bool(valid.any())
    if kind == 'edges':
        assert sorted(set(valid.sum(1).tolist())) == list(range(13))
    fk, Wg, gw = kw_inputs(rng, m, tab.K, G, H)
    got, r32, r64, _ = kw_check(fk, Wg, tab, G, H, gw, (2e-6, 6e-6, 2e-6))
    if kind == 'none':                                                   # exact: nothing is added anywhere
        for k in ('w', 'dfk', 'dW'):
            assert torch.equal(got[k], torch.zeros_like(got[k])), k
        from crfconv_amd.graph import table_from_edges
        no = torch.empty(0, dtype=torch.long, device=DEV)
        got = kw_run(fk, Wg, table_from_edges(no, no, m, m), G, H, gw[:, :1].contiguous())      # E = 0: one column of -1
        for k in ('w', 'dfk', 'dW'):
            assert torch.equal(got[k], torch.zeros_like(got[k])), k
    if kind == 'self':                                                   # exact: e = 1, the weight is the fp32 sum of Wg in kernel order
        s = np.float32(0)
        for g in range(G):
            s = np.float32(s + Wg[g].numpy())
        loops = rows == torch.arange(m)[:, None]
        assert bool((got['w'][loops] == float(s)).all())
    empty = ~valid.any(1) & (indeg == 0)
    assert torch.equal(got['dfk'][empty], torch.zeros_like(got['dfk'][empty]))  # exact: no edge on either side
    if kind == 'hub':
        for k, b in (('dfk', 6e-6), ('dW', 2e-6)):
            assert not rejected(got[k], r32[k], r64[k], b)
        bent = got['dfk'].double().clone()
        bent[5] -= r64['dfk_src'][5]                                     # the hub row's reverse walk left out
        assert rejected(bent, r32['dfk'], r64['dfk'], 6e-6)
        assert rejected(got['dfk'].double() - 2.0 * r64['dfk_src'], r32['dfk'], r64['dfk'], 6e-6)   # the source-side term with the wrong sign
        assert rejected(got['dW'].double() * (1.0 + 10.0 * 2e-6), r32['dW'], r64['dW'], 2e-6)
        assert rejected(got['w'].double() * (1.0 + 10.0 * 2e-6), r32['w'], r64['w'], 2e-6)


def test_kernel_weights_only_self_loops_are_exact():
    """Every entry a self-loop or a hole: distance 0, e = 1 -- the weight is exactly sum_g Wg[g], every feature gradient exactly 0 and
    dW[g] = sum of gw over the loops (the kernel sums fp32 values in float64: exact, then one rounding to fp32)."""
    m, K, G, H = 301, 9, 5, 64
    rng = np.random.default_rng(11)
    rows = np.tile(np.arange(m)[:, None], (1, K))
    rows[rng.random((m, K)) < 0.3] = -1
    tab = index_table(rows)
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    got = kw_run(fk, Wg, tab, G, H, gw)
    s = np.float32(0)
    for g in range(G):
        s = np.float32(s + Wg[g].numpy())
    valid = device_rows(tab) >= 0
    assert torch.equal(got['w'], torch.where(valid, torch.tensor(float(s)), torch.tensor(0.0)))
    assert torch.equal(got['dfk'], torch.zeros_like(got['dfk']))
    assert torch.equal(got['dW'], gw.double()[valid].sum().float().expand(G).contiguous())


# ------------------------------------------------------------------ (e) numeric edges
def test_kernel_weights_signs_and_zero_in_Wg():
    """Wg = (-0.7, 0, 0.9): the weight is a difference of two kernels, the zero kernel still gets its dW.
    Bounds: w 4e-6, dfk 2e-6, dW 2e-6 (CPU float32 restatement: 4.0e-7 / 8.5e-8 / 9.3e-8).
    Measured on the MI355X: w 3.6e-7, dfk 1.3e-7, dW 2.7e-8."""
    m, K, G, H = 301, 9, 3, 64
    rng = np.random.default_rng(21)
    tab = index_table(shaped_rows('holes', rng, m, K))
    fk, _, gw = kw_inputs(rng, m, K, G, H)
    Wg = torch.tensor([-0.7, 0.0, 0.9])
    got, _, r64, _ = kw_check(fk, Wg, tab, G, H, gw, (4e-6, 2e-6, 2e-6))
    assert float(got['dW'][1].abs()) > 0.1 * float(r64['dW'].abs().max())


def test_kernel_weights_underflowing_distances_give_exact_zeros():
    """Two clusters of feature rows 1.5 apart in each of 64 channels: every cross-cluster distance is above 110 and expf(-d) is 0 in
    fp32.  Columns 0 .. 3 stay inside the cluster, columns 4 .. 8 cross: the weight is exactly 0 there, and with a gradient on the cross
    entries alone both gradients are exact zeros; everything is finite.
    Bounds: w 2e-6, dfk 2e-6, dW 2e-6 (CPU float32 restatement: 1.6e-7 / 1.0e-7 / 9.2e-8).
    Measured on the MI355X: w 1.3e-7, dfk 1.3e-7, dW 5.1e-8."""
    m, K, G, H = 301, 9, 5, 64
    rng = np.random.default_rng(31)
    half = m // 2
    rows = np.empty((m, K), dtype=np.int64)
    rows[:half, :4], rows[:half, 4:] = rng.integers(0, half, (half, 4)), rng.integers(half, m, (half, 5))
    rows[half:, :4], rows[half:, 4:] = rng.integers(half, m, (m - half, 4)), rng.integers(0, half, (m - half, 5))
    tab = index_table(rows)
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    fk[half:] += 1.5
    f64 = fk.double().view(m, G, H)
    d = ((f64[torch.from_numpy(rows[:, 4:])] - f64[:, None]) ** 2).sum(-1)
    assert float(d.min()) > 110.0
    got, _, _, _ = kw_check(fk, Wg, tab, G, H, gw, (2e-6, 2e-6, 2e-6))
    assert torch.equal(got['w'][:, 4:], torch.zeros(m, 5))
    gw_cross = gw.clone()
    gw_cross[:, :4] = 0.0
    got = kw_run(fk, Wg, tab, G, H, gw_cross)
    for k in ('dfk', 'dW'):
        assert torch.equal(got[k], torch.zeros_like(got[k])), k


def test_kernel_weights_identical_feature_rows():
    """Every row of fk the same vector: e = 1 on every edge, the feature gradient exactly 0, dW[g] the sum of gw over the valid entries."""
    m, K, G, H = 301, 9, 5, 64
    rng = np.random.default_rng(41)
    tab = index_table(shaped_rows('holes', rng, m, K))
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    fk = fk[:1].expand(m, G * H).contiguous()
    got = kw_run(fk, Wg, tab, G, H, gw)
    valid = device_rows(tab) >= 0
    assert torch.equal(got['dfk'], torch.zeros_like(got['dfk']))
    assert torch.equal(got['dW'], gw.double()[valid].sum().float().expand(G).contiguous())
    assert bool((got['w'][valid] == got['w'][valid][0]).all()) and bool((got['w'][~valid] == 0).all())


def test_kernel_weights_gradient_scale():
    """gw x 1e3 and x 1e-3: every gradient is linear in gw, so its error on its own scale stays where it was -- it moves by no more than
    one float32 restatement's error (the rounding is re-drawn, not amplified).
    Bounds: dfk 7e-6, dW 2e-6 at every scale (CPU float32 restatement, largest of the three scales: 6.8e-7 / 8.5e-8).
    Largest measured on the MI355X: dfk 7.5e-7, dW 5.0e-8."""
    m, K, G, H = 301, 9, 5, 64
    rng = np.random.default_rng(51)
    tab = index_table(shaped_rows('hub', rng, m, K))
    rows = device_rows(tab)
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    seen = {}
    for s in (1.0, 1e3, 1e-3):
        g = gw * np.float32(s)
        r64 = kw_reference(fk, Wg, rows, G, H, g, torch.float64)
        r32 = kw_reference(fk, Wg, rows, G, H, g, torch.float32)
        got = kw_run(fk, Wg, tab, G, H, g)
        seen[s] = {k: own_scale(got[k], r32[k], r64[k], b, '%s x%g' % (k, s)) for k, b in (('dfk', 7e-6), ('dW', 2e-6))}
    for s in (1e3, 1e-3):
        for k in ('dfk', 'dW'):
            (e, e32), (e1, e321) = seen[s][k], seen[1.0][k]
            assert abs(e - e1) <= max(abs(e32 - e321), e32, e321), '%s: own-scale error %.3e at gw x %g, %.3e at x 1' % (k, e, s, e1)


def test_kernel_weights_non_contiguous_and_partial_grads():
    """fk and gw as strided views (through _f32c): bit for bit what the contiguous tensors give.  Only Wg, or only fk, requiring grad:
    the same values for the one that does, None for the other."""
    m, K, G, H = 301, 9, 5, 64
    rng = np.random.default_rng(61)
    tab = index_table(shaped_rows('holes', rng, m, K))
    fk, Wg, gw = kw_inputs(rng, m, K, G, H)
    base = kw_run(fk, Wg, tab, G, H, gw)
    wide_f = torch.zeros(m, 2 * G * H)
    wide_f[:, ::2] = fk
    wide_g = torch.zeros(K, m)
    wide_g[:] = gw.t()

    from crfconv_amd import ops
    fd = dev(wide_f)[:, ::2].requires_grad_(True)
    Wd = dev(Wg).requires_grad_(True)
    assert not fd.is_contiguous()
    w = ops.kernel_weights(fd, Wd, tab, G, H)
    gd = dev(wide_g).t()
    assert not gd.is_contiguous()
    poison(fk.shape, fk.shape, gw.shape)
    w.backward(gd)
    assert torch.equal(w.detach().cpu(), base['w']) and torch.equal(fd.grad.cpu(), base['dfk']) and torch.equal(Wd.grad.cpu(), base['dW'])

    only_w = kw_run(fk, Wg, tab, G, H, gw, fk_grad=False)
    assert only_w['dfk'] is None and torch.equal(only_w['dW'], base['dW'])
    only_f = kw_run(fk, Wg, tab, G, H, gw, W_grad=False)
    assert only_f['dW'] is None and torch.equal(only_f['dfk'], base['dfk'])


# ------------------------------------------------------------------ (f) refusals
def test_kernel_weights_refusals():
    """G = 9, H = 257, K = 65 and a CPU tensor raise CrfConvError in front of the first launch (the library's argument check, require_gpu)."""
    from crfconv_amd import ops
    from crfconv_amd._lib import CrfConvError
    m = 12
    rng = np.random.default_rng(0)
    tab = index_table(rng.integers(0, m, (m, 4)))
    for G, H, msg in ((9, 4, 'num_kernels=9'), (1, 257, 'hidden_channels=257')):
        with pytest.raises(CrfConvError, match=msg):
            ops.kernel_weights(torch.zeros(m, G * H, device=DEV), torch.ones(G, device=DEV), tab, G, H)
    with pytest.raises(CrfConvError, match='K=65'):
        ops.kernel_weights(torch.zeros(m, 8, device=DEV), torch.ones(2, device=DEV), index_table(rng.integers(0, m, (m, 65))), 2, 4)
    with pytest.raises(CrfConvError, match='no CPU path'):
        ops.kernel_weights(torch.zeros(m, 8), torch.ones(2, device=DEV), tab, 2, 4)
    with pytest.raises(CrfConvError, match='no CPU path'):
        ops.kernel_weights(torch.zeros(m, 8, device=DEV), torch.ones(2), tab, 2, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (g) weighted_step
def ws_reference(x, z, w, Q, P, rows, gout, dtype):
    leaves = [leaf(v, dtype) for v in (x, z, w, Q, P)]
    out = ref_weighted_step(*leaves, rows)
    (out * gout.to(dtype)).sum().backward()
    return dict(out=out.detach(), **{'d' + k: v.grad for k, v in zip('xzwQP', leaves)})


def ws_run(x, z, w, Q, P, tab, gout, need='xzwQP'):
    from crfconv_amd import ops
    leaves = {k: dev(v).requires_grad_(k in need) for k, v in zip('xzwQP', (x, z, w, Q, P))}
    poison(x.shape)
    out = ops.weighted_step(*leaves.values(), tab)
    poison(x.shape, x.shape, x.shape, w.shape, x.shape, Q.shape, Q.shape)   # gm, mt, dx, dw, dz, dQ, dP
    out.backward(dev(gout))
    res = dict(out=out.detach().cpu())
    for k, v in leaves.items():
        assert (v.grad is not None) == (k in need), k
        res['d' + k] = None if v.grad is None else v.grad.cpu()
    return res


@pytest.mark.parametrize('H,K,kind', [(4, 9, 'hub'), (8, 1, 'holes'), (16, 16, 'dense'), (32, 64, 'empty'), (64, 9, 'hub'), (64, 16, 'holes'),
                                      (4, 64, 'dup'), (8, 16, 'empty'), (16, 9, 'ragged'), (32, 16, 'dup'), (64, 1, 'holes'), (64, 64, 'ragged')])
def test_weighted_step(H, K, kind):
    """crfconv_meanfield_step / _bwd_edge / _bwd_scatter with given weights at every compiled width H in (4, 8, 16, 32, 64), K = 1, 9, 16
    (where the continuous path takes its fast kernels and this entry must not: a dense NeighborTable and padded ones) and 64, m = 301.
    Q and P are general non-symmetric matrices (dz = G Q^T, dQ = z^T G, dP = mt^T G: a missing transpose shows), the weights have either
    sign and exact zeros, and the value 7 on missing entries, which nothing may read: dw is exactly 0 there.  A second pass with only x,
    or only w, requiring grad gives the same bits.  hub: bent results are refused.
    Bounds: out 3e-6, dx 4e-6, dz 3e-6, dw 2e-6, dQ 7e-6, dP 9e-6 (CPU float32 restatement, largest of the 12 cases: 2.5e-7, 3.5e-7, 3.4e-7,
    2.1e-7, 6.8e-7, 8.7e-7).  Largest measured on the MI355X: out 3.1e-7, dx 4.5e-7, dz 3.0e-7, dw 2.4e-7, dQ 2.6e-7, dP 2.9e-7."""
    m = 301
    rng = np.random.default_rng(100 * H + K)
    tab = dense_table(rng.integers(0, m, (m, K))) if kind == 'dense' else index_table(shaped_rows(kind, rng, m, K))
    rows = device_rows(tab)
    valid = rows >= 0
    x, z, gout = (torch.from_numpy(rng.standard_normal((m, H)).astype(np.float32)) for _ in range(3))
    Q, P = (torch.from_numpy((rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32)) for _ in range(2))
    w = torch.from_numpy(rng.standard_normal((m, K)).astype(np.float32))
    w[torch.from_numpy(rng.random((m, K)) < 0.1)] = 0.0
    w[~valid] = 7.0
    assert bool((w[valid] < 0).any()) and bool((w[valid] > 0).any()) and bool((w[valid] == 0).any()) or K == 1
    r64 = ws_reference(x, z, w, Q, P, rows, gout, torch.float64)
    r32 = ws_reference(x, z, w, Q, P, rows, gout, torch.float32)
    got = ws_run(x, z, w, Q, P, tab, gout)
    bounds = dict(out=3e-6, dx=4e-6, dz=3e-6, dw=2e-6, dQ=7e-6, dP=9e-6)
    for k, b in bounds.items():
        own_scale(got[k], r32[k], r64[k], b, k)
    assert torch.equal(got['dw'][~valid], torch.zeros(int((~valid).sum())))          # exact
    indeg = torch.bincount(rows[valid], minlength=m)
    assert torch.equal(got['dx'][indeg == 0], torch.zeros(int((indeg == 0).sum()), H))   # exact: an empty reverse row
    for need in ('x', 'w'):
        part = ws_run(x, z, w, Q, P, tab, gout, need=need)
        assert torch.equal(part['d' + need], got['d' + need]) and torch.equal(part['out'], got['out'])
    if kind == 'hub':
        for k, b in bounds.items():
            assert not rejected(got[k], r32[k], r64[k], b), k
        bent = got['dx'].double().clone()
        bent[5] -= r64['dx'][5]                                          # the hub row's reverse walk left out
        assert rejected(bent, r32['dx'], r64['dx'], 4e-6)
        assert rejected(-got['dx'].double(), r32['dx'], r64['dx'], 4e-6)
        assert rejected(got['dQ'].double().t(), r32['dQ'], r64['dQ'], 7e-6)
        assert rejected(got['dP'].double().t(), r32['dP'], r64['dP'], 9e-6)
        assert rejected(got['dP'].double() * (1.0 + 10.0 * 9e-6), r32['dP'], r64['dP'], 9e-6)
        G64 = gout.double()
        assert rejected(got['dz'].double() - G64 @ Q.double().t() + G64 @ Q.double(), r32['dz'], r64['dz'], 3e-6)   # dz = G Q, not G Q^T
        assert rejected(got['dw'].double() * (1.0 + 10.0 * 2e-6), r32['dw'], r64['dw'], 2e-6)


def test_weighted_step_refusals():
    """xout aliasing xin and a width outside (4, 8, 16, 32, 64) are refused by the raw library entry in front of the launch; CPU tensors
    by the operator."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    m, K = 12, 4
    tab = index_table(np.random.default_rng(0).integers(0, m, (m, K)))
    x, z, out = (torch.zeros(m, 16, device=DEV) for _ in range(3))
    w = torch.zeros(m, K, device=DEV)
    Q = torch.eye(16, device=DEV)
    lib = _lib.load()
    assert lib.crfconv_meanfield_step(ptr(x), ptr(z), ptr(w), ptr(tab.idx32), K, 0, m, 16, ptr(Q), ptr(Q), ptr(x), stream_ptr()) == -1
    assert b'alias' in lib.crfconv_last_error()
    assert lib.crfconv_meanfield_step(ptr(x), ptr(z), ptr(w), ptr(tab.idx32), K, 0, m, 12, ptr(Q), ptr(Q), ptr(out), stream_ptr()) == -3
    assert b'H=12' in lib.crfconv_last_error()
    with pytest.raises(_lib.CrfConvError):
        ops.weighted_step(torch.zeros(m, 12, device=DEV), torch.zeros(m, 12, device=DEV), w, torch.eye(12, device=DEV), torch.eye(12, device=DEV), tab)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        ops.weighted_step(x.cpu(), z, w, Q, Q, tab)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (h) discrete_meanfield
def dm_case(rng, m, K, L, scale):
    rows = shaped_rows('empty', rng, m, K)
    logits = f32(rng, (m, L), -scale, scale)
    p = torch.softmax(logits, -1)
    w = f32(rng, (m, K), -0.3, 0.7)
    w[torch.from_numpy(rows < 0)] = 7.0
    C = torch.eye(L) + torch.from_numpy((0.3 * rng.standard_normal((L, L))).astype(np.float32))
    C[0, 1], C[1, 0] = -C[0, 1].abs(), C[1, 0].abs()
    assert bool((C[~torch.eye(L, dtype=torch.bool)] < 0).any()) and bool((C[~torch.eye(L, dtype=torch.bool)] > 0).any())
    gout = torch.from_numpy(rng.standard_normal((m, L)).astype(np.float32))
    return rows, p, w, C, gout


def dm_reference(p, w, C, rows, steps, gout, dtype):
    leaves = [leaf(v, dtype) for v in (p, w, C)]
    q = ref_discrete_meanfield(*leaves, rows, steps)
    (q * gout.to(dtype)).sum().backward()
    return dict(q=q.detach(), dp=leaves[0].grad, dw=leaves[1].grad, dC=leaves[2].grad)


def dm_run(p, w, C, tab, steps, gout):
    from crfconv_amd import ops
    pd, wd, Cd = (dev(v).requires_grad_(True) for v in (p, w, C))
    q = ops.discrete_meanfield(pd, -torch.log(pd), wd, Cd, tab, steps)
    poison(p.shape, w.shape)
    (q * gout.to(DEV)).sum().backward()
    return dict(q=q.detach().cpu(), dp=pd.grad.cpu(), dw=wd.grad.cpu(), dC=Cd.grad.cpu())


@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('L', [2, 3, 4, 5, 8, 9, 13, 16, 17, 32, 33, 64])
def test_discrete_meanfield_label_counts(L, steps):
    """Every padded width of _CRF_H = (4, 8, 16, 32, 64): L equal to a width (4, 8, 16, 32, 64: no padding), one above a width (5, 9, 17,
    33: maximal padding) and between (2, 3, 13); C with off-diagonal entries of both signs, weights of both signs, p from logits in +-2.
    The padding columns stay out of the soft-max: q has L columns, its rows sum to 1, and it equals the reference, which knows no
    padding.  A row without a valid entry keeps q = p.  m = 203, K = 7, holes anywhere.
    Bounds: q 2e-6, dp 6e-6, dw 3e-6, dC 1e-5 (CPU float32 restatement, largest of the 24 cases: 2.4e-7, 5.6e-7, 3.0e-7, 1.25e-6).
    Largest measured on the MI355X: q 1.2e-6, dp 3.0e-6, dw 1.6e-6, dC 1.1e-6, all at L = 64.  The kernel's error grows with the padded
    width (q: 1.9e-7 at 8, 3.3e-7 at 16, 7.1e-7 at 32, 1.2e-6 at 64) where the restatement's does not: step_kernel adds the H products of
    msg P onto z Q -- the large term, -u -- one fma at a time, H roundings at the size of u; the restatement rounds there once
    (that order replayed in torch float32 on this test's data: 1.3e-7, 2.4e-7, 6.1e-7, 1.1e-6; with z added last 1.4e-7 .. 2.1e-7)."""
    m, K = 203, 7
    rng = np.random.default_rng(10 * L + steps)
    rows, p, w, C, gout = dm_case(rng, m, K, L, 2.0)
    tab = index_table(rows)
    rows = device_rows(tab)
    r64 = dm_reference(p, w, C, rows, steps, gout, torch.float64)
    r32 = dm_reference(p, w, C, rows, steps, gout, torch.float32)
    got = dm_run(p, w, C, tab, steps, gout)
    assert got['q'].shape == (m, L)
    for k, b in (('q', 2e-6), ('dp', 6e-6), ('dw', 3e-6), ('dC', 1e-5)):
        own_scale(got[k], r32[k], r64[k], b, k)
    assert float((got['q'].sum(1) - 1.0).abs().max()) <= 4 * 1.1920929e-07 * max(1.0, np.log2(L))   # fp32 rounding of a sum of L terms
    empty = ~(rows >= 0).any(1)
    assert int(empty.sum()) >= 3 and torch.allclose(got['q'][empty], p[empty], rtol=0, atol=1e-6)
    assert torch.equal(got['dw'][rows < 0], torch.zeros(int((rows < 0).sum())))      # exact


def test_discrete_meanfield_near_one_hot():
    """p from logits in +-12: u = -log p reaches ~24 and most of q's entries are far below its largest.  L = 13, steps = 3.
    Bounds from the float32 restatement at THIS input (CPU: q 1.9e-7, dp 1.04e-6, dw 2.6e-7, dC 3.6e-7): q 2e-6, dp 1e-5, dw 3e-6, dC 4e-6.
    Measured on the MI355X: q 1.6e-7, dp 2.3e-6, dw 3.8e-7, dC 2.2e-7."""
    m, K, L, steps = 203, 7, 13, 3
    rng = np.random.default_rng(1212)
    rows, p, w, C, gout = dm_case(rng, m, K, L, 12.0)
    assert float((-torch.log(p)).max()) > 16.0
    tab = index_table(rows)
    rows = device_rows(tab)
    r64 = dm_reference(p, w, C, rows, steps, gout, torch.float64)
    r32 = dm_reference(p, w, C, rows, steps, gout, torch.float32)
    got = dm_run(p, w, C, tab, steps, gout)
    for k, b in (('q', 2e-6), ('dp', 1e-5), ('dw', 3e-6), ('dC', 4e-6)):
        own_scale(got[k], r32[k], r64[k], b, k)
    assert float((got['q'].sum(1) - 1.0).abs().max()) <= 16 * 1.1920929e-07


def test_discrete_meanfield_no_steps_and_too_many_labels():
    """steps = 0 returns p itself; 65 labels exceed the widest kernel and are refused."""
    from crfconv_amd import ops
    from crfconv_amd._lib import CrfConvError
    m, K = 12, 4
    tab = index_table(np.random.default_rng(0).integers(0, m, (m, K)))
    w = torch.zeros(m, K, device=DEV)
    p = torch.softmax(torch.randn(m, 5, generator=torch.Generator().manual_seed(0)), -1).to(DEV)
    assert ops.discrete_meanfield(p, -torch.log(p), w, torch.eye(5, device=DEV), tab, 0) is p
    p = torch.full((m, 65), 1.0 / 65, device=DEV)
    with pytest.raises(CrfConvError):
        ops.discrete_meanfield(p, -torch.log(p), w, torch.eye(65, device=DEV), tab, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (i) the three operators chained, against the oracle
def test_operator_chain_against_the_oracle():
    """ops.linear -> kernel_weights -> discrete_meanfield as DiscreteCRFConv chains them, on one ragged table_from_edges table at
    (G, H, L, steps) = (8, 200, 17, 2) -- HPL = 4 and the padded label width 32, which no module test reaches -- against
    oracle.discrete_crf in float64 on the device's edge order: q and the gradients of the logits, f, F, W and C.
    Bounds: q 2e-6, dlogit 2e-6, df 5e-6, dF 6e-6, dW 6e-6, dC 6e-6 (CPU float32 oracle: 1.3e-7, 1.8e-7, 4.7e-7, 6.1e-7, 6.4e-7, 6.3e-7).
    Measured on the MI355X: q 2.5e-7, dlogit 4.4e-7, df 1.4e-6, dF 6.7e-7, dW 2.6e-7, dC 5.2e-7."""
    from crfconv_amd import ops
    from oracle import crf_oracle as O
    n, D, G, H, L, steps = 257, 6, 8, 200, 17, 2
    rng = np.random.default_rng(8200)
    tab = edges_table(rng, n, tuple(range(13)))
    rows = device_rows(tab)
    valid = rows >= 0
    tgt, src = torch.nonzero(valid)[:, 0], rows[valid]
    inputs = dict(logit=f32(rng, (n, L), -2, 2), f=f32(rng, (n, D), 0, 1), F=f32(rng, (G, D, H), 0, 0.1),
                  W=f32(rng, (G, 1), 0.2, 0.5) * torch.where(torch.arange(G) % 3 == 1, -0.3, 1.0)[:, None],
                  C=torch.eye(L) + torch.from_numpy((0.3 * rng.standard_normal((L, L))).astype(np.float32)))
    gout = torch.from_numpy(rng.standard_normal((n, L)).astype(np.float32))

    def oracle(dtype):
        v = {k: leaf(a, dtype) for k, a in inputs.items()}
        q = O.discrete_crf(v, '', torch.softmax(v['logit'], -1), v['f'], tgt, src, steps)
        (q * gout.to(dtype)).sum().backward()
        return dict(q=q.detach(), **{'d' + k: a.grad for k, a in v.items()})
    r64, r32 = oracle(torch.float64), oracle(torch.float32)

    v = {k: dev(a).requires_grad_(True) for k, a in inputs.items()}
    p = torch.softmax(v['logit'], -1)
    fk = ops.linear(v['f'], v['F'].permute(0, 2, 1).reshape(G * H, D))
    w = ops.kernel_weights(fk, v['W'].reshape(-1), tab, G, H)
    q = ops.discrete_meanfield(p, -torch.log(p), w, v['C'], tab, steps)
    poison((n, G * H), (n, G * H), (n, tab.K), (n, 32))
    (q * gout.to(DEV)).sum().backward()
    own_scale(q, r32['q'], r64['q'], 2e-6, 'q')
    bounds = dict(logit=2e-6, f=5e-6, F=6e-6, W=6e-6, C=6e-6)
    for k in inputs:
        own_scale(v[k].grad, r32['d' + k], r64['d' + k], bounds[k], 'd' + k)
    dF = v['F'].grad.double().cpu()
    assert rejected(dF * (1.0 + 10.0 * 6e-6), r32['dF'], r64['dF'], 6e-6)
