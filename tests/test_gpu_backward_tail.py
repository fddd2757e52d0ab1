"""-m gpu: the end-of-backward parameter pass of the wide PointConv layers on the matrix pipe (csrc/pointconv_wide_params.hip; shared
steps: csrc/pointconv_wide.hpp), driven through crfconv_pointconv_wide_params_jobs and the slab sums directly: d = 128 (a pair of
wavefronts per target point) and d = 32 / 64 (one wavefront per point) against a float64 restatement on the edge list, the three widths
in one launch against one launch each, and a d = 128 layer against the dump path."""
import functools

import pytest
import torch

from gpu_util import DEV, assert_close

pytestmark = pytest.mark.gpu
GRAD_TOL = 2e-4
K, SLOPE = 16, 0.1


@functools.lru_cache(maxsize=None)
def _case(d, m_tgt, n_src, ragged, seed):
    """Inputs of one parameter pass (CPU float32) and its float64 results.  Source and target points are disjoint random sets (no
    rel = 0); ragged: in-degrees 3 .. 16 on a padded table with entries < 0, the construction of
    test_pointconv_wide_layers_on_a_padded_table_with_missing_edges."""
    g = torch.Generator().manual_seed(seed)
    if ragged:
        deg = torch.randint(3, 17, (m_tgt,), generator=g)
        deg[7] = 16
    else:
        deg = torch.full((m_tgt,), K, dtype=torch.int64)
    idx = torch.full((m_tgt, K), -1, dtype=torch.int32)
    for i, k in enumerate(deg.tolist()):
        idx[i, :k] = torch.randperm(n_src, generator=g)[:k].int()
    pos_s, pos_t = torch.rand(n_src, 3, generator=g), torch.rand(m_tgt, 3, generator=g)
    x, gout = torch.randn(n_src, d, generator=g), torch.randn(m_tgt, d, generator=g)
    A1, b1, W2 = torch.randn(d, 3, generator=g), torch.randn(d, generator=g), torch.randn(d, d, generator=g) / d ** 0.5
    ca, cb, cc = (torch.rand(d, generator=g) - 0.5 for _ in range(3))
    inp = dict(d=d, m_tgt=m_tgt, idx=idx, pos_s=pos_s, pos_t=pos_t, x=x, gout=gout, A1=A1, b1=b1, W2=W2, ca=ca, cb=cb, cc=cc)
    # float64 on the edge list
    tgt, slot = torch.nonzero(idx >= 0, as_tuple=True)
    src = idx[tgt, slot].long()
    D = lambda v: v.double()
    rel = D(pos_t)[tgt] - D(pos_s)[src]
    pre = rel @ D(A1).t() + D(b1)
    h1 = torch.where(pre > 0, pre, SLOPE * pre)
    h2 = h1 @ D(W2).t()
    gh2 = D(ca) * (D(gout)[tgt] * D(x)[src]) + D(cb) * h2 + D(cc)
    dW2 = gh2.t() @ h1
    gp = (gh2 @ D(W2)) * torch.where(pre > 0, 1.0, SLOPE)
    dA1b1 = gp.t() @ torch.cat([rel, torch.ones(len(rel), 1, dtype=torch.float64)], 1)
    return inp, dW2, dA1b1, float(pre.abs().min())


def _job(inp):
    """(PcWideJob, slabs dW2 [nblk, d d] float, slabs dA1 | db1 [nblk, 4 d] float64, nblk, tensors to keep alive); slabs start as NaN."""
    from crfconv_amd import _lib
    lib = _lib.load()
    d, m = inp['d'], inp['m_tgt']
    assert lib.crfconv_pointconv_wide_params_supported(m, K, d) == 1
    nb = int(lib.crfconv_pointconv_wide_params_nblk(m, d))
    dev = {k: inp[k].to(DEV).contiguous() for k in ('x', 'gout', 'pos_s', 'pos_t', 'idx', 'A1', 'b1', 'W2', 'ca', 'cb', 'cc')}
    pw = torch.full((nb, d * d), float('nan'), dtype=torch.float32, device=DEV)
    pa = torch.full((nb, 4 * d), float('nan'), dtype=torch.float64, device=DEV)
    job = _lib.PcWideJob(dev['x'].data_ptr(), dev['gout'].data_ptr(), dev['pos_s'].data_ptr(), dev['pos_t'].data_ptr(), dev['idx'].data_ptr(),
                         K, m, d, dev['A1'].data_ptr(), dev['b1'].data_ptr(), dev['W2'].data_ptr(), SLOPE, dev['ca'].data_ptr(),
                         dev['cb'].data_ptr(), dev['cc'].data_ptr(), pw.data_ptr(), pa.data_ptr())
    return job, pw, pa, nb, dev


def _run(jobs):
    from crfconv_amd import _lib
    from crfconv_amd.graph import stream_ptr
    _lib.call('crfconv_pointconv_wide_params_jobs', (_lib.PcWideJob * len(jobs))(*jobs), len(jobs), stream_ptr())


def _check_vs_float64(d, m_tgt, n_src, ragged, seed):
    """One pass of width d alone: its slabs summed by the batched sum entries, dW2 and dA1 | db1 against the float64 of _case."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import stream_ptr
    inp, dW2, dA1b1, margin = _case(d, m_tgt, n_src, ragged, seed)
    assert margin > 1e-5, 'seed %d puts a layer-1 pre-activation %.3e from the kink' % (seed, margin)
    if ragged:
        assert bool((inp['idx'] < 0).any())
    job, pw, pa, nb, keep = _job(inp)
    _run([job])
    gw = torch.empty(d * d, dtype=torch.float32, device=DEV)
    ga = torch.empty(4 * d, dtype=torch.float64, device=DEV)
    _lib.call('crfconv_reduce_jobs', (_lib.ReduceJob * 1)(_lib.ReduceJob(pw.data_ptr(), gw.data_ptr(), nb, d * d)), 1, stream_ptr())
    _lib.call('crfconv_reduce_jobs_f64', (_lib.Reduce64Job * 1)(_lib.Reduce64Job(pa.data_ptr(), 0, nb, 4 * d, ga.data_ptr())), 1, stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pw).all()) and bool(torch.isfinite(pa).all()), 'a slab was left unwritten'
    assert_close(gw.view(d, d), dW2, GRAD_TOL, 'dW2')
    assert_close(ga.view(d, 4), dA1b1, GRAD_TOL, 'dA1|db1')


@pytest.mark.parametrize('m_tgt,n_src,ragged,seed', [(1, 40, False, 3), (9, 40, False, 1), (333, 517, True, 6)],
                         ids=['one-point', 'nine-points', 'ragged-333'])
def test_wide_params_d128_vs_float64(m_tgt, n_src, ragged, seed):
    """dW2 and dA1 | db1 of the d = 128 pass, summed over its slabs by the batched sum entries, against float64: one point (three pairs
    of the workgroup idle), nine (an odd count over the pairs of a workgroup), 333 on a padded ragged table (a count no partition
    divides: a short last workgroup).  No pre-activation of the float64 reference lies within 1e-5 of the LeakyReLU kink, so nothing is masked out."""
    _check_vs_float64(128, m_tgt, n_src, ragged, seed)


@pytest.mark.parametrize('d,m_tgt,n_src,ragged,seed',
                         [(32, 1, 40, False, 3), (64, 1, 40, False, 3), (32, 9, 40, False, 1), (64, 9, 40, False, 1),
                          (32, 333, 517, True, 6), (64, 333, 517, True, 7)],
                         ids=['32-one-point', '64-one-point', '32-nine-points', '64-nine-points', '32-ragged-333', '64-ragged-333'])
def test_wide_params_d32_d64_vs_float64(d, m_tgt, n_src, ragged, seed):
    """The same for the one-wavefront-per-point pass of d = 32 and 64: one point (seven of the eight wavefronts idle), nine (two workgroups
    of five and four points, idle wavefronts in both), 333 on a padded ragged table (42 workgroups, a short last one).  Margins of the float64 reference from
    the kink (asserted > 1e-5): 2.3e-3 / 3.4e-3, 1.7e-5 / 3.9e-5, 3.6e-5 (seed 6) / 1.95e-5 (seed 7; seed 6 gives 3.5e-6 at d = 64)."""
    _check_vs_float64(d, m_tgt, n_src, ragged, seed)


def test_wide_params_three_widths_in_one_call_match_one_call_each():
    """Jobs of d = 128, 64 and 32 in one launch (handed over narrowest first: the entry orders them) leave, per job, the slabs of the
    same job launched alone, bit for bit."""
    cases = [_case(32, 50, 64, False, 5)[0], _case(128, 9, 40, False, 1)[0], _case(64, 37, 64, True, 6)[0]]
    together = [_job(c) for c in cases]
    _run([j[0] for j in together])
    alone = [_job(c) for c in cases]
    for j in alone:
        _run([j[0]])
    torch.cuda.synchronize()
    for c, a, b in zip(cases, together, alone):
        assert bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(a[2]).all()), 'd = %d: a slab was left unwritten' % c['d']
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), 'd = %d' % c['d']


def test_d128_matrix_pipe_pass_reproduces_the_dump_path():
    """A d = 128 layer of the benchmarked level (640 points, K = 16) under deferred weight gradients: the matrix-pipe pass forms its
    products in the summation orders of the passes it replaces (layer 2 as the vector kernels' ascending chain, g_h2 W2 in gemm_tile's k
    order, dW2 over the weight-gradient pass's row slices and wavefronts, dA1 | db1 from float products in float64), so every parameter
    gradient equals the dump + GEMM path's (ops.state.no_wide128) bit for bit -- a training run does not move."""
    from torch import nn
    from crfconv_amd import ops
    from crfconv_amd.graph import table_from_edges
    d, n = 128, 640
    g = torch.Generator().manual_seed(24)
    tgt = torch.repeat_interleave(torch.arange(n), K)
    src = torch.cat([torch.randperm(n, generator=g)[:K] for _ in range(n)])
    pos_s, pos_t = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    x0, gout = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    W1_0, W2_0 = torch.randn(d, 3, generator=g), torch.randn(d, d, generator=g) / d ** 0.5
    gam1, bet1, gam2, bet2 = (torch.rand(d, generator=g) + 0.5 for _ in range(4))
    table = table_from_edges(tgt.to(DEV), src.to(DEV), n, n)
    assert table.K == K

    def run(no_wide128):
        W1, W2 = nn.Parameter(W1_0.to(DEV)), nn.Parameter(W2_0.to(DEV))
        bn1, bn2 = nn.BatchNorm1d(d).to(DEV).train(), nn.BatchNorm1d(d).to(DEV).train()
        with torch.no_grad():
            bn1.weight.copy_(gam1); bn1.bias.copy_(bet1); bn2.weight.copy_(gam2); bn2.bias.copy_(bet2)
        x = x0.to(DEV).requires_grad_(True)
        out = ops.point_conv(x, pos_s.to(DEV), pos_t.to(DEV), table, W1, bn1, W2, bn2, True)
        was = ops.state.no_wide128
        ops.state.no_wide128 = no_wide128
        try:
            with ops.deferred_weight_grads():
                (out * gout.to(DEV)).sum().backward()
        finally:
            ops.state.no_wide128 = was
        return [v.grad.clone() for v in (W1, W2, bn1.weight, bn1.bias, bn2.weight, bn2.bias)]
    for a, b, name in zip(run(False), run(True), ('dW1', 'dW2', 'dgamma1', 'dbeta1', 'dgamma2', 'dbeta2')):
        assert bool(a.abs().max() > 0) and torch.equal(a, b), name
