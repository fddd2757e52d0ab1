"""-m gpu: the job-table forms of the row-streaming MLP kernels (csrc/linear_fwd.hpp linear_fwd_jobs_kernel, csrc/mlp_bwd.hip
mlp_bwd_p1_jobs_kernel) and the node that uses them (ops.mlp._MLPStreamGroup).

The contract is bit-identity per job with the single launches: crfconv_linear_forward_jobs against crfconv_linear_forward (y and the
statistic records), both followed by crfconv_bn_apply_from_records(_jobs) (out, coef, the running statistics); crfconv_mlp_backward_jobs
against crfconv_mlp_backward / _add (dX, dgamma, dbeta, the workspace slabs, and dW finished from them by crfconv_mlp_dw_jobs).  Every
comparison is torch.equal.  The single launches of every shape run ONCE (`singles`) and are left unchanged.

Shapes (M, Ci, Co): (301, 8, 8) -- a partial 16-row group, NCH = 1; (1237, 32, 8) -- NCH = 2; (33 000, 64, 16) -- more than 512 x 64 rows,
so the grid-stride sweep runs with the JOB's block count, NCH = 4; (40, 16, 16).  Calls of 1, 2 and 4 jobs, and two job orders.  In the
backward, job (1237, 32, 8) has an addend (the dX form with EPI_ADD, TCO = 2), job (40, 16, 16) has dX = NULL, all have dW = NULL; every
call is made twice in a row on the same ticket words, which must be left zero.

"Equal" must not mean "equally wrong": one two-job call of each direction is also checked against the float64 evaluation of
test_gpu_mlp_stream.block_reference on the CPU, with the bounds that module uses for the same quantities (BOUNDS_F64 below names
their origin), its inputs, its nudge of beta away from the LeakyReLU kink and its asserted margin TAU.

Module level: a ContinuousGaussianCRFConv(64, 32, steps=3) in training mode, N = 2048, N' = 512, with ops.state.mfma_min_rows lowered
to 256 so that both embeddings take the streaming family -- output, input gradients and every parameter gradient with the groups on
against ops.state.no_stream_groups = True, torch.equal, and the grouped run must really have gone through the group node.  The same with
the switch-over between the two row counts: the mixed pair, whose tiled member's product (crf_linear_job.tiled; at the library level one
500 x 128 -> 16 job against crfconv_gemm_stats beside one 2000 x 64 -> 16 job) rides the streaming member's forward launch."""

import numpy as np
import pytest
import torch

from gpu_util import DEV
from test_gpu_discrete import dev, own_scale
from test_gpu_mlp_stream import EPS, MOM, TAU, make_inputs, prepare
from test_gpu_pointconv import seed

pytestmark = pytest.mark.gpu

SHAPES = ((301, 8, 8), (1237, 32, 8), (33000, 64, 16), (40, 16, 16))
ADD_JOB, NO_DX_JOB = 1, 3
CALLS = ((0,), (1, 2), (0, 1, 2, 3), (3, 2, 1, 0), (2, 1))           # 1, 2 and 4 jobs; two orders of the four and of a pair
SLOPE = 0.1

# Copied from tests/test_gpu_mlp_stream.py BOUNDS (10 x the float32 restatement's error on the CPU, see there): 'fork_and_mask' -- a block
# whose dX takes an alias gradient -- for the job with the addend, 'block_widths' for the job without.
BOUNDS_F64 = {
    True: dict(rm=2e-06, rv=2e-06, out=4e-06, dx=5e-06, dW=6e-06, dgamma=3e-06, dbeta=2e-06),
    False: dict(rm=2e-06, rv=1e-06, out=6e-06, dx=6e-06, dW=7e-06, dgamma=8e-06, dbeta=2e-06),
}


def lib_():
    from crfconv_amd import _lib
    return _lib


def P(t):
    return None if t is None else t.data_ptr()


def empty(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


@pytest.fixture(scope='module')
def inputs():
    """Per shape the host inputs of test_gpu_mlp_stream.make_inputs (nudged: prepare), their two references, and the device copies."""
    out = []
    for i, (m, ci, co) in enumerate(SHAPES):
        inp = make_inputs('block', seed(31, m, ci, co), m, ci, co, slope=SLOPE, galias=(i == ADD_JOB), want_dx=(i != NO_DX_JOB), fork=True)
        r32, r64 = prepare(inp)                                # asserts min |pre-activation| >= TAU in float64
        assert r64['_pre_min'] >= TAU
        d = {k: dev(v) for k, v in inp.items() if torch.is_tensor(v)}
        out.append(dict(inp=inp, r32=r32, r64=r64, d=d, m=m, ci=ci, co=co))
    return out


def forward_buffers(s):
    m, co = s['m'], s['co']
    nrec = lib_().load().crfconv_linear_forward_stat_records(m)
    return dict(y=empty(m, co), rec=empty(nrec, 4, co), out=empty(m, co), coef=empty(4 * co), rm=s['d']['rm'].clone(), rv=s['d']['rv'].clone(),
                nrec=nrec)


def forward_jobs(ss, bufs):
    _lib = lib_()
    n = len(ss)
    lf = (_lib.LinearJob * n)()
    ba = (_lib.BnApplyJob * n)()
    for i, (s, b) in enumerate(zip(ss, bufs)):
        d = s['d']
        lf[i] = _lib.LinearJob(P(d['x']), P(d['W']), s['m'], s['ci'], s['co'], P(b['y']), P(b['rec']))
        ba[i] = _lib.BnApplyJob(P(b['rec']), b['nrec'], P(b['y']), s['m'], s['co'], P(d['g']), P(d['b']), P(b['rm']), P(b['rv']), MOM, EPS, None,
                                SLOPE, P(b['coef']), P(b['out']))
    _lib.call('crfconv_linear_forward_jobs', lf, n, None)
    _lib.call('crfconv_bn_apply_from_records_jobs', ba, n, None)
    torch.cuda.synchronize()


def backward_buffers(s, i):
    m, ci, co = s['m'], s['ci'], s['co']
    nbytes = lib_().load().crfconv_mlp_backward_workspace(m, ci, co)
    return dict(dx=None if i == NO_DX_JOB else empty(m, ci), dgamma=empty(co), dbeta=empty(co), dW=empty(co, ci),
                ws=torch.zeros(nbytes, dtype=torch.uint8, device=DEV), nbytes=nbytes)


def finish_dw(ss, fwd, bufs):
    """dW of every job from its workspace slabs: crfconv_mlp_dw_jobs."""
    _lib = lib_()
    jobs = (_lib.MlpDwJob * len(ss))(*[_lib.MlpDwJob(P(b['ws']), P(f['coef']), P(b['dW']), s['m'], s['ci'], s['co']) for s, f, b in zip(ss, fwd, bufs)])
    _lib.call('crfconv_mlp_dw_jobs', jobs, len(ss), None)
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def tickets():
    n = lib_().load().crfconv_ticket_bytes() // 4
    return dict(one=torch.zeros(n, dtype=torch.int32, device=DEV), group=torch.zeros(4 * n, dtype=torch.int32, device=DEV))


@pytest.fixture(scope='module')
def singles(inputs, tickets):
    """The single launches of every shape, once: forward product with records, coefficients + apply, backward, dW."""
    _lib = lib_()
    res = []
    for i, s in enumerate(inputs):
        d = s['d']
        m, ci, co = s['m'], s['ci'], s['co']
        assert _lib.load().crfconv_linear_forward_jobs_supported(m, ci, co) == 1 and _lib.load().crfconv_mlp_backward_p1_jobs_supported(m, ci, co) == 1 \
            and _lib.load().crfconv_mlp_backward_dx_jobs_supported(m, ci, co) == 1
        f = forward_buffers(s)
        _lib.call('crfconv_linear_forward', P(d['x']), P(d['W']), None, m, ci, co, 0, P(f['y']), P(f['rec']), None)
        _lib.call('crfconv_bn_apply_from_records', P(f['rec']), f['nrec'], P(f['y']), m, co, P(d['g']), P(d['b']), P(f['rm']), P(f['rv']), MOM, EPS,
                  None, SLOPE, P(f['coef']), P(f['out']), None)
        b = backward_buffers(s, i)
        tail = (None, P(b['dgamma']), P(b['dbeta']), P(b['ws']), b['nbytes'], P(tickets['one']), None)
        head = (P(d['gout']), P(f['y']), P(d['x']), P(d['W']), P(f['coef']), SLOPE, m, ci, co)
        if i == ADD_JOB:
            _lib.call('crfconv_mlp_backward_add', *head, P(d['galias']), P(b['dx']), *tail)
        else:
            _lib.call('crfconv_mlp_backward', *head, P(b['dx']), *tail)
        torch.cuda.synchronize()
        finish_dw([s], [f], [b])
        res.append((f, b))
    assert int(tickets['one'].abs().max()) == 0
    return res


def run_backward_jobs(ss, idx, fwd, tickets):
    _lib = lib_()
    bufs = [backward_buffers(s, i) for s, i in zip(ss, idx)]
    jobs = (_lib.MlpStreamBwdJob * len(ss))()
    for k, (s, i, f, b) in enumerate(zip(ss, idx, fwd, bufs)):
        d = s['d']
        jobs[k] = _lib.MlpStreamBwdJob(P(d['gout']), P(f['y']), P(d['x']), P(d['W']), P(f['coef']), SLOPE, s['m'], s['ci'], s['co'],
                                       P(d['galias']) if i == ADD_JOB else None, P(b['dx']), None, P(b['dgamma']), P(b['dbeta']), P(b['ws']), b['nbytes'])
    _lib.call('crfconv_mlp_backward_jobs', jobs, len(ss), P(tickets['group']), None)
    torch.cuda.synchronize()
    finish_dw(ss, fwd, bufs)
    return bufs


@pytest.mark.parametrize('call', CALLS, ids=lambda c: '-'.join(map(str, c)))
def test_forward_jobs_equal_the_single_launches(call, inputs, singles):
    ss = [inputs[i] for i in call]
    bufs = [forward_buffers(s) for s in ss]
    forward_jobs(ss, bufs)
    for i, b in zip(call, bufs):
        ref = singles[i][0]
        for k in ('y', 'rec', 'out', 'coef', 'rm', 'rv'):
            assert torch.equal(b[k], ref[k]), 'job of shape %s in call %s: %s differs from the single launch' % (SHAPES[i], call, k)
        assert bool(torch.isfinite(b['out']).all())


@pytest.mark.parametrize('call', CALLS, ids=lambda c: '-'.join(map(str, c)))
def test_backward_jobs_equal_the_single_launches(call, inputs, singles, tickets):
    ss = [inputs[i] for i in call]
    fwd = [singles[i][0] for i in call]
    first = run_backward_jobs(ss, call, fwd, tickets)
    assert int(tickets['group'].abs().max()) == 0, 'ticket words not left zero'
    second = run_backward_jobs(ss, call, fwd, tickets)             # on the ticket words the first call left behind
    assert int(tickets['group'].abs().max()) == 0
    for i, b1, b2 in zip(call, first, second):
        ref = singles[i][1]
        for k in ('dx', 'dgamma', 'dbeta', 'ws', 'dW'):
            if ref[k] is None:
                assert b1[k] is None and i == NO_DX_JOB
                continue
            assert torch.equal(b1[k], ref[k]), 'job of shape %s in call %s: %s differs from the single launch' % (SHAPES[i], call, k)
            assert torch.equal(b2[k], b1[k]), 'job of shape %s in call %s: %s differs between two calls in a row' % (SHAPES[i], call, k)
        assert bool(torch.isfinite(b1['dW']).all()) and bool(torch.isfinite(b1['dgamma']).all())


def test_a_two_job_call_of_each_direction_against_float64(inputs, tickets):
    """Jobs (301, 8, 8) and (1237, 32, 8, with the addend) in one call each way, every tensor against float64 on its own scale."""
    call = (0, 1)
    ss = [inputs[i] for i in call]
    fwd = [forward_buffers(s) for s in ss]
    forward_jobs(ss, fwd)
    bwd = run_backward_jobs(ss, call, fwd, tickets)
    for i, s, f, b in zip(call, ss, fwd, bwd):
        assert s['r64']['_pre_min'] >= TAU                         # the margin from the LeakyReLU kink, in float64
        got = dict(out=f['out'], rm=f['rm'], rv=f['rv'], dx=b['dx'], dW=b['dW'], dgamma=b['dgamma'], dbeta=b['dbeta'])
        assert set(got) == set(k for k in s['r64'] if not k.startswith('_'))
        for k, g in sorted(got.items()):
            own_scale(g, s['r32'][k], s['r64'][k], BOUNDS_F64[i == ADD_JOB][k], 'job %d.%s' % (i, k))


def test_limits_are_refused(inputs, tickets):
    _lib = lib_()
    lib = _lib.load()
    assert lib.crfconv_linear_forward_jobs_supported(1000, 32, 32) == 0          # two output tiles: TCO = 2
    assert lib.crfconv_linear_forward_jobs_supported(1000, 128, 16) == 0         # eight k chunks
    assert lib.crfconv_linear_forward_jobs_supported(1000, 6, 8) == 0            # not a multiple of 4
    assert lib.crfconv_mlp_backward_p1_jobs_supported(1000, 32, 32) == 0 and lib.crfconv_mlp_backward_dx_jobs_supported(1000, 32, 32) == 0
    assert lib.crfconv_mlp_backward_p1_jobs_supported(1000, 32, 12) == 0         # no last-workgroup channel part at Co = 12
    s = inputs[0]
    f = forward_buffers(s)
    job = (_lib.LinearJob * 5)(*[_lib.LinearJob(P(s['d']['x']), P(s['d']['W']), s['m'], s['ci'], s['co'], P(f['y']), P(f['rec']))] * 5)
    assert lib.crfconv_linear_forward_jobs(job, 5, None) < 0 and lib.crfconv_linear_forward_jobs(job, 0, None) < 0
    bad = (_lib.LinearJob * 1)(_lib.LinearJob(P(s['d']['x']), P(s['d']['W']), s['m'], 8, 32, P(f['y']), P(f['rec'])))
    assert lib.crfconv_linear_forward_jobs(bad, 1, None) < 0
    torch.cuda.synchronize()


def test_a_tiled_job_rides_the_streaming_launch(inputs):
    """The mixed pair: one tiled job (500 x 128 -> 16, the product of crfconv_gemm_stats) as the first workgroups of the launch of one
    row-streaming job (2000 x 64 -> 16) -- y and the records of both equal the single entry points', bit for bit."""
    _lib = lib_()
    lib = _lib.load()
    rng = seed(31, 500, 2000)
    shapes = ((500, 128, 16), (2000, 64, 16))
    x = [dev(0.5 + torch.from_numpy(rng.standard_normal((m, ci)).astype(np.float32))) for m, ci, _ in shapes]
    W = [dev(torch.from_numpy((rng.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32))) for _, ci, co in shapes]
    nrec = [lib.crfconv_gemm_stat_records(500), lib.crfconv_linear_forward_stat_records(2000)]
    assert lib.crfconv_linear_forward_jobs_tiled_supported(*shapes[0]) == 1 and lib.crfconv_linear_forward_jobs_supported(*shapes[1]) == 1

    def buffers():
        return [(empty(m, co), empty(n, co, 4)) for (m, _, co), n in zip(shapes, nrec)]
    ref, got = buffers(), buffers()
    (m, ci, co), (y, rec) = shapes[0], ref[0]
    _lib.call('crfconv_gemm_stats', P(x[0]), P(W[0]), m, co, ci, P(y), P(rec), None)
    (m, ci, co), (y, rec) = shapes[1], ref[1]
    _lib.call('crfconv_linear_forward', P(x[1]), P(W[1]), None, m, ci, co, 0, P(y), P(rec), None)
    jobs = (_lib.LinearJob * 2)(*[_lib.LinearJob(P(x[k]), P(W[k]), shapes[k][0], shapes[k][1], shapes[k][2], P(got[k][0]), P(got[k][1]), 1 - k)
                                  for k in range(2)])
    _lib.call('crfconv_linear_forward_jobs', jobs, 2, None)
    torch.cuda.synchronize()
    for k, what in enumerate(('tiled', 'streaming')):
        assert bool(torch.isfinite(got[k][0]).all()) and bool(torch.isfinite(got[k][1]).all()), what
        assert torch.equal(got[k][0], ref[k][0]), '%s job: y differs from the single entry point' % what
        assert torch.equal(got[k][1], ref[k][1]), '%s job: the statistic records differ from the single entry point' % what
    # the tiled jobs come first, and need a row-streaming job to ride on
    swapped = (_lib.LinearJob * 2)(jobs[1], jobs[0])
    assert lib.crfconv_linear_forward_jobs(swapped, 2, None) < 0 and lib.crfconv_linear_forward_jobs(jobs, 1, None) < 0
    torch.cuda.synchronize()


def crf_layer_run(grouped, min_rows=256, one_launch=True):
    """Forward and backward of the layer with the groups on or off, from the same seeded state: output, input and parameter gradients."""
    from crfconv_amd import models, ops
    from crfconv_amd.ops import mlp as opsmlp
    rng = seed(31, 2048, 512)
    B, N, Nc, K = 1, 2048, 512, 8
    state = torch.get_rng_state()
    torch.default_generator.manual_seed(7)                     # the same initial parameters in both runs; the generator's state is put back
    try:
        layer = models.ContinuousGaussianCRFConv(64, 32, steps=3).to(DEV).train()
    finally:
        torch.set_rng_state(state)
    unary = torch.from_numpy(rng.standard_normal((B, Nc, 64)).astype(np.float32)).to(DEV).requires_grad_(True)
    pairwise = torch.from_numpy(rng.standard_normal((B, N, 32)).astype(np.float32)).to(DEV).requires_grad_(True)
    up_idx = torch.from_numpy(rng.integers(0, Nc, (B, N, 1))).to(DEV)
    nbr = rng.integers(0, N, (B, N, K))
    nbr[:, :, 0] = np.arange(N)[None]
    neighbor_idx = torch.from_numpy(nbr).to(DEV)
    gout = torch.from_numpy(rng.standard_normal((B, N, 32)).astype(np.float32)).to(DEV)
    keep_rows, keep_off, keep_small = ops.state.mfma_min_rows, ops.state.no_stream_groups, ops.state.small_mlp_disabled
    before = opsmlp._MLPStreamGroup.calls
    try:
        ops.state.mfma_min_rows = min_rows
        ops.state.no_stream_groups = not grouped
        ops.state.small_mlp_disabled = keep_small or not one_launch
        out = layer(unary, pairwise, up_idx, neighbor_idx)
        out.backward(gout)
        torch.cuda.synchronize()
    finally:
        ops.state.mfma_min_rows, ops.state.no_stream_groups, ops.state.small_mlp_disabled = keep_rows, keep_off, keep_small
    took = opsmlp._MLPStreamGroup.calls - before
    res = dict(out=out.detach().clone(), d_unary=unary.grad.clone(), d_pairwise=pairwise.grad.clone())
    for name, p in layer.named_parameters():
        assert p.grad is not None, name
        res['d ' + name] = p.grad.clone()
    for name, b in layer.named_buffers():
        res['buffer ' + name] = b.detach().clone()
    return res, took


def test_crf_layer_with_the_groups_equals_without():
    on, took_on = crf_layer_run(True)
    off, took_off = crf_layer_run(False)
    assert took_on == 2 and took_off == 0, 'group node forwards: %d with the groups (the two stages of the embeddings), %d without' % (took_on, took_off)
    assert set(on) == set(off)
    for k in sorted(on):
        assert bool(torch.isfinite(on[k].float()).all()), k
        assert torch.equal(on[k], off[k]), '%s differs between the grouped and the one-by-one run' % k


def test_crf_layer_with_the_mixed_groups_equals_without():
    """The switch-over at 1024 rows, the one-launch coarse kernel off: unary_nn (512 rows) runs the tiled product, pairwise_nn (2048 rows) the
    row-streaming one -- the mixed pair in one forward launch, the members' own backward paths."""
    on, took_on = crf_layer_run(True, min_rows=1024, one_launch=False)
    off, took_off = crf_layer_run(False, min_rows=1024, one_launch=False)
    assert took_on == 2 and took_off == 0, 'group node forwards: %d with the groups, %d without' % (took_on, took_off)
    assert set(on) == set(off)
    for k in sorted(on):
        assert bool(torch.isfinite(on[k].float()).all()), k
        assert torch.equal(on[k], off[k]), '%s differs between the grouped and the one-by-one run' % k
