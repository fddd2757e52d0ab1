"""-m gpu: optim.FlatAdam / FlatAdamW (csrc/optim.hip: adam_sqnorm_kernel, adam_prologue_kernel, adam_update_kernel) against
torch.optim.Adam / AdamW, and through train.CapturedStep and the self-capturing forward.

Bound of every comparison against torch: ``assert_close_anchored(got, ref32, ref64, 1e-6)`` -- `got` the device result, `ref64` / `ref32`
torch's optimizer on the CPU in float64 / float32 fed the same gradients (``clip_grad_norm_`` in front where clipping is on): 1e-6 of
the largest value (FlatSGD's bound), or 4 x torch's own float32 error where that is larger.  An off-by-one step count or a swapped bias
correction is an error of the order of lr (1e-2 here).

Misaligned operands at the C entry (test_misaligned_views_...): the implementation's choice is the CORRECT ELEMENT-BY-ELEMENT PATH, not
CRF_ERR_ARG -- views at an odd element offset give the bits of the aligned call."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _seeded as S
from gpu_util import DEV, assert_close, assert_close_anchored, t

pytestmark = pytest.mark.gpu

LR = 1e-2
BIG = 2 * 2048 * 256 * 4 + 5          # two full sweeps of the capped grid (2048 workgroups x 256 lanes x float4) and a ragged tail


def small_net():
    return torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.BatchNorm1d(33), torch.nn.Linear(33, 5))


class Vecs(torch.nn.Module):
    """Bare parameters of the given sizes."""

    def __init__(self, values):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(v.clone()) for v in values])


def torch_adam(params, cfg, lr=LR):
    cfg = dict(cfg)
    cfg.pop('grad_scale', None), cfg.pop('max_grad_norm', None)
    return torch.optim.Adam(params, lr=lr, **cfg)


def cpu_twins(module):
    """(float32, float64) CPU copies of a device module."""
    out = []
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(module).cpu().to(dt)
        out.append(m)
    return out


def feed(refs, grads, scale=1.0, max_norm=None):
    """.grad of the CPU twins <- scale * grads (in their dtype), clipped as the reference loop would."""
    for r in refs:
        ps = list(r.parameters())
        for p, g in zip(ps, grads):
            p.grad = (g.detach().cpu() * scale).to(p.dtype)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)


def close_to_refs(net, refs, what):
    for (k, a), b32, b64 in zip(net.named_parameters(), refs[0].parameters(), refs[1].parameters()):
        assert_close_anchored(a, b32, b64, 1e-6, '%s %s' % (what, k))


# ------------------------------------------------------------------ 1. against torch, small net
@pytest.mark.parametrize('cfg', [dict(), dict(weight_decay=1e-2), dict(weight_decay=1e-2, decoupled_weight_decay=True),
                                 dict(betas=(0.8, 0.99), eps=1e-6, amsgrad=True), dict(grad_scale=0.5)],
                         ids=['defaults', 'coupled_wd', 'adamw', 'betas_eps_amsgrad', 'grad_scale'])
def test_flat_adam_matches_torch_adam(cfg):
    """Four steps on the three-layer net of test_flat_sgd_matches_torch_sgd, same seeded gradients, parameters compared after every
    step.  grad_scale = 0.5: the reference is fed halved gradients.  AdamW goes through the FlatAdamW class."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    torch.manual_seed(3)
    net = small_net().to(DEV)
    refs = cpu_twins(net)
    before = [p.detach().clone() for p in net.parameters()]
    bucket = FlatGradAllReduce(net)
    if cfg.get('decoupled_weight_decay'):
        opt = optim.FlatAdamW(bucket, lr=LR, weight_decay=cfg['weight_decay'])
    else:
        opt = optim.FlatAdam(bucket, lr=LR, **cfg)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    ropts = [torch_adam(r.parameters(), cfg) for r in refs]
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), before))                 # re-homing kept the values
    assert net[0].weight.data_ptr() == opt.flat.data_ptr()
    for step in range(4):
        grads = [t(S.uniform(step, 'g%d' % i, tuple(p.shape))) for i, p in enumerate(net.parameters())]
        for v, g in zip(bucket.views, grads):
            v.copy_(g)
        feed(refs, grads, cfg.get('grad_scale', 1.0))
        opt.step()
        for o in ropts:
            o.step()
        close_to_refs(net, refs, 'step %d' % step)
    assert int(opt.t) == 4 and opt.steps == 4


def test_flat_adam_rejects_invalid_hyper_parameters():
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            optim.FlatAdam(FlatGradAllReduce(torch.nn.Linear(3, 2).to(DEV)), **bad)


# ------------------------------------------------------------------ 2. sizes at which the kernel can go wrong
@pytest.mark.parametrize('n,amsgrad', [(1, False), (3, True), (1023, False), (1025, True), (BIG, False), (BIG, True)])
def test_flat_adam_sizes_every_element(n, amsgrad):
    """One flat parameter of n elements, 3 steps, EVERY element compared: below one lane, tail only, around one workgroup sweep with
    n % 4 != 0, and past two full sweeps of the capped grid (the grid-stride loop wraps, ragged tail).  Elements whose gradient is
    exactly zero in every step must not move (weight_decay = 0)."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    gen = torch.Generator().manual_seed(n)
    p0 = torch.rand(n, generator=gen) * 2 - 1
    zero = (torch.arange(n) % 7) == 3
    net = Vecs([p0]).to(DEV)
    refs = cpu_twins(net)
    bucket = FlatGradAllReduce(net)
    opt = optim.FlatAdam(bucket, lr=LR, amsgrad=amsgrad)
    ropts = [torch_adam(r.parameters(), dict(amsgrad=amsgrad)) for r in refs]
    for step in range(3):
        g = torch.rand(n, generator=gen) * 2 - 1
        g[zero] = 0.0
        bucket.flat.copy_(g)
        feed(refs, [g])
        opt.step()
        for o in ropts:
            o.step()
    close_to_refs(net, refs, 'n=%d after 3 steps' % n)
    assert torch.equal(opt.flat.cpu()[zero], p0[zero])
    assert int(opt.t) == 3


# ------------------------------------------------------------------ 3. misaligned C entry
def _c_step(p, g, m, v, x, hyper, clip=False):
    """crfconv_adam_step on raw vectors (no guard words); returns grad_norm."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    lib = _lib.load()
    n = p.numel()
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    coef = torch.zeros(int(lib.crfconv_adam_coef_floats()), dtype=torch.float32, device=DEV)
    norm = torch.zeros((), dtype=torch.float32, device=DEV)
    ws = torch.zeros(int(lib.crfconv_adam_workspace(n)) // 8, dtype=torch.float64, device=DEV)
    h = torch.tensor(hyper, dtype=torch.float64).to(DEV)
    _lib.call('crfconv_adam_step', ptr(p), ptr(g), ptr(m), ptr(v), ptr(x), n, ptr(h), ptr(step), ptr(coef), ptr(norm), 0, 1 if clip else 0,
              ptr(ws), ws.numel() * 8, None, 0, None, stream_ptr())
    torch.cuda.synchronize()
    assert int(step) == 1
    return norm


def test_misaligned_views_at_the_c_entry_take_the_element_path_and_give_equal_bits():
    """``flat[1:]``-style views of ALL operand vectors (4 bytes past a 16-byte boundary), n = 1027: the entry takes its element-by-element
    path, which must give the bits of the float4 path on the same values (parameters, both moments, the amsgrad maximum).  With clipping
    the misaligned norm pass sums in another order: its norm is held to the bound of the aligned one (1e-6 of the float64 norm)."""
    n = 1027
    gen = torch.Generator().manual_seed(5)
    vals = [torch.rand(n, generator=gen) * s + o for s, o in ((2, -1), (2, -1), (2, -1), (1, 0), (1, 0.5))]     # p, g, m, v >= 0, vmax > 0
    hyper = (LR, 0.9, 0.999, 1e-8, 1e-2, 0.5, 1.0, 0.0)
    aligned = [x.to(DEV) for x in vals]
    holders = [torch.zeros(n + 1, device=DEV) for _ in vals]
    views = [h[1:] for h in holders]
    for w, x in zip(views, vals):
        w.copy_(x)
    assert all(a.data_ptr() % 16 == 0 for a in aligned) and all(w.data_ptr() % 16 == 4 for w in views)
    _c_step(*aligned, hyper)
    _c_step(*views, hyper)
    for name, a, w, x in zip(('param', 'grad', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'), aligned, views, vals):
        assert torch.equal(a, w), name
        assert torch.equal(a.cpu(), x) == (name == 'grad'), name                 # everything but the gradient was updated
    assert all(float(h[0]) == 0.0 for h in holders)                              # nothing written in front of the views
    n64 = float((vals[1].double() * 0.5).norm())
    for vecs in (aligned, views):                                                # (a second step on the same vectors: the gradient is as it was)
        norm = float(_c_step(*vecs, hyper, clip=True))
        assert abs(norm - n64) <= 1e-6 * n64, (norm, n64)


# ------------------------------------------------------------------ 4. clipping
@pytest.mark.parametrize('max_norm', [1.0, 1000.0], ids=['below_the_norm', 'above_the_norm'])
def test_flat_adam_global_norm_clipping(max_norm):
    """max_grad_norm below and above the gradient norm (about 77 for 71 028 uniform gradients halved by grad_scale; 70 workgroup
    partials): opt.grad_norm is the unclipped float64 norm to 1e-6, parameters follow clip_grad_norm_ + Adam, two runs from equal state
    give equal bits, and step() leaves the bucket as it was (the coefficient is applied inside the update)."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    sizes = (70001, 1027)
    gen = torch.Generator().manual_seed(9)
    p0 = [torch.rand(s, generator=gen) * 2 - 1 for s in sizes]
    grads = [[torch.rand(s, generator=gen) * 2 - 1 for s in sizes] for _ in range(3)]
    refs = cpu_twins(Vecs(p0))
    ropts = [torch_adam(r.parameters(), dict(weight_decay=1e-2)) for r in refs]

    def run():
        net = Vecs(p0).to(DEV)
        bucket = FlatGradAllReduce(net)
        opt = optim.FlatAdam(bucket, lr=LR, weight_decay=1e-2, max_grad_norm=max_norm, grad_scale=0.5)
        norms, after = [], []
        for gs in grads:
            for v, g in zip(bucket.views, gs):
                v.copy_(g)
            kept = bucket.flat.clone()
            opt.step()
            assert torch.equal(bucket.flat, kept)
            norms.append(opt.grad_norm.clone())
            after.append(opt.flat.clone())
        return net, norms, after
    net, norms, after = run()
    for step, gs in enumerate(grads):
        n64 = float(torch.cat([g.double() * 0.5 for g in gs]).norm())
        assert (n64 > max_norm) == (max_norm == 1.0)
        assert abs(float(norms[step]) - n64) <= 1e-6 * n64, (step, float(norms[step]), n64)
        feed(refs, gs, 0.5, max_norm)
        for o in ropts:
            o.step()
        flat32, flat64 = (torch.cat([p.detach().reshape(-1) for p in r.parameters()]) for r in refs)
        assert_close_anchored(after[step], flat32, flat64, 1e-6, 'step %d' % step)
    _, norms2, after2 = run()
    assert all(torch.equal(a, b) for a, b in zip(norms + after, norms2 + after2))


# ------------------------------------------------------------------ 5. capture, scheduler, device counter
def test_flat_adam_follows_exponential_lr_scheduler_eager_and_captured():
    """Two eager steps, then ONE captured step replayed three times, ExponentialLR(gamma=0.5) and push_hyper() between the steps, against
    torch Adam stepped five times.  A step count frozen at capture, or advanced by the warm-up step in front of the capture, is an
    error of the order of lr; the device counter reads 5 at the end."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    torch.manual_seed(2)
    net = torch.nn.Linear(6, 4).to(DEV)
    refs = cpu_twins(net)
    bucket = FlatGradAllReduce(net)
    opt = optim.FlatAdam(bucket, lr=0.05, weight_decay=1e-3)
    ropts = [torch_adam(r.parameters(), dict(weight_decay=1e-3), lr=0.05) for r in refs]
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    rschs = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.5) for o in ropts]
    graph = None
    for step in range(5):
        grads = [t(S.uniform(step, 'h%d' % i, tuple(p.shape))) for i, p in enumerate(net.parameters())]
        for v, g in zip(bucket.views, grads):
            v.copy_(g)
        feed(refs, grads)
        if step < 2:
            opt.step()
        else:
            if graph is None:                                 # capture ONE step; the following ones are replays
                snap, sd = opt.flat.clone(), opt.state_dict()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    opt.step()                                # a warm-up step, undone below
                torch.cuda.current_stream().wait_stream(side)
                opt.load_state_dict(sd)
                with torch.no_grad():
                    opt.flat.copy_(snap)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()
                assert int(opt.t) == 2 and opt.steps == 2     # a capture runs nothing and counts nothing
            graph.replay()
        for o in ropts:
            o.step()
        sch.step()
        for s_ in rschs:
            s_.step()
        opt.push_hyper()
        assert abs(opt.lr - ropts[0].param_groups[0]['lr']) < 1e-12
        close_to_refs(net, refs, 'step %d' % step)
    assert int(opt.t) == 5


# ------------------------------------------------------------------ 6. guard
def test_flat_adam_skips_the_update_while_the_barrier_failure_word_is_set():
    """After a healthy step the sticky failure word is set (a word written by the host: nothing is provoked on the device) and the
    bucket holds NaN: three eager steps and one replay must leave parameters, both moments, the amsgrad maximum and t untouched;
    check_gridsync raises; the next step is finite, moves the parameters and advances t by exactly one."""
    from crfconv_amd import _lib, ops, optim
    from crfconv_amd.distributed import FlatGradAllReduce
    dev = torch.device('cuda', 0)
    torch.manual_seed(4)
    net = torch.nn.Linear(9, 17).to(DEV)
    bucket = FlatGradAllReduce(net)
    opt = optim.FlatAdam(bucket, lr=0.1, weight_decay=1e-4, amsgrad=True, max_grad_norm=1.0, check_every=0)
    ws = ops.gridsync_ws(dev)
    # the word a failing CAPTURED kernel sets lives in the device's capture buffer: a replayed step always watches that one and its own
    # stream's, other streams' only while the device has at most 8 barrier workspaces (ops.fail_word_ptrs)
    from crfconv_amd.ops import _base
    cap = _base._sync_ws[(dev.index, 'capture')]
    ops.check_gridsync(dev)
    word = _lib.load().crfconv_gridsync_fail_word()
    was = ops.state.small_mlp_disabled
    try:
        bucket.flat.fill_(1.0)
        opt.step()                                           # a healthy step first: the moments are non-zero afterwards
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
        state = lambda: [x.clone() for x in (opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq, opt.t)]      # noqa: E731
        s0 = state()
        assert int(opt.t) == 1 and float(opt.exp_avg.abs().max()) > 0
        ws[word] = 0x101
        cap[word] = 0x101
        bucket.flat.fill_(float('nan'))                      # what a poisoned forward / backward leaves behind
        for _ in range(3):
            opt.step()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(state(), s0))
        with pytest.raises(_lib.CrfConvError, match='grid barrier timed out'):
            ops.check_gridsync(dev)
        assert int(ws[word]) == 0 and int(cap[word]) == 0
        bucket.flat.fill_(1.0)
        opt.step()                                           # word cleared: the update runs again, from intact state
        torch.cuda.synchronize()
        assert bool(torch.isfinite(opt.flat).all()) and not torch.equal(opt.flat, s0[0])
        assert int(opt.t) == 2
    finally:
        ws.zero_(), cap.zero_()                              # (a failed assertion above must not leave the words set for later tests)
        ops.state.small_mlp_disabled = was


# ------------------------------------------------------------------ 7. state round trips
def _seeded_grads(net, step, key='s'):
    return [t(S.uniform(step, '%s%d' % (key, i), tuple(p.shape))) for i, p in enumerate(net.parameters())]


def test_flat_adam_resumes_a_torch_adam_run():
    """torch Adam (float32, amsgrad) for 2 steps, load_torch_state into a FlatAdam over the same parameter values, 2 further steps on
    both; a torch state whose `step` differs between parameters raises ValueError."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    cfg = dict(weight_decay=1e-2, amsgrad=True)
    torch.manual_seed(6)
    net = small_net().to(DEV)
    refs = cpu_twins(net)
    ropts = [torch_adam(r.parameters(), cfg) for r in refs]
    for step in range(2):
        feed(refs, _seeded_grads(net, step))
        for o in ropts:
            o.step()
    with torch.no_grad():
        for p, r in zip(net.parameters(), refs[0].parameters()):
            p.copy_(r)
    bucket = FlatGradAllReduce(net)
    opt = optim.FlatAdam(bucket, lr=LR, **cfg)
    sd = ropts[0].state_dict()
    opt.load_torch_state(sd)
    assert int(opt.t) == 2
    for step in range(2, 4):
        grads = _seeded_grads(net, step)
        for v, g in zip(bucket.views, grads):
            v.copy_(g)
        feed(refs, grads)
        opt.step()
        for o in ropts:
            o.step()
        close_to_refs(net, refs, 'resumed step %d' % step)
    uneven = copy.deepcopy(sd)
    uneven['state'][1]['step'] = uneven['state'][1]['step'] + 1
    with pytest.raises(ValueError, match='step'):
        opt.load_torch_state(uneven)


def test_torch_adam_resumes_a_flat_adam_run_and_flat_state_dict_round_trip():
    """FlatAdam for 2 steps; torch_state_dict() loaded into fresh torch Adams (float32 / float64) over the same parameter values, one
    step on all: they agree.  state_dict() / load_state_dict() into a second FlatAdam reproduces that step bit for bit."""
    from crfconv_amd import optim
    from crfconv_amd.distributed import FlatGradAllReduce
    cfg = dict(weight_decay=1e-2, amsgrad=True)
    torch.manual_seed(7)
    net = small_net().to(DEV)
    bucket = FlatGradAllReduce(net)
    opt = optim.FlatAdam(bucket, lr=LR, **cfg)
    for step in range(2):
        for v, g in zip(bucket.views, _seeded_grads(net, step)):
            v.copy_(g)
        opt.step()
    tsd = opt.torch_state_dict()
    assert all(float(st['step']) == 2.0 for st in tsd['state'].values()) and len(tsd['state']) == len(bucket.params)
    refs = cpu_twins(net)
    ropts = [torch_adam(r.parameters(), dict(), lr=123.0) for r in refs]       # (hyper-parameters come from the loaded group)
    for o in ropts:
        o.load_state_dict(copy.deepcopy(tsd))
        assert o.param_groups[0]['lr'] == LR and o.param_groups[0]['amsgrad'] is True
    net2 = copy.deepcopy(net)
    bucket2 = FlatGradAllReduce(net2)
    opt2 = optim.FlatAdam(bucket2, lr=LR, **cfg)
    opt2.load_state_dict(opt.state_dict())
    assert int(opt2.t) == 2 and opt2.steps == 2
    grads = _seeded_grads(net, 2)
    for b in (bucket, bucket2):
        for v, g in zip(b.views, grads):
            v.copy_(g)
    feed(refs, grads)
    opt.step(), opt2.step()
    for o in ropts:
        o.step()
    close_to_refs(net, refs, 'torch resumed')
    for a, b in ((opt.flat, opt2.flat), (opt.exp_avg, opt2.exp_avg), (opt.exp_avg_sq, opt2.exp_avg_sq),
                 (opt.max_exp_avg_sq, opt2.max_exp_avg_sq), (opt.t, opt2.t)):
        assert torch.equal(a, b)
    assert opt2.flat.data_ptr() != opt.flat.data_ptr()


# ------------------------------------------------------------------ 8. / 9. the dense network: CapturedStep and the self-capturing forward
B, N = 2, 8192


@pytest.fixture(scope='module')
def batches():
    import test_gpu_autograph as AG                        # its batch builder: B = 2 clouds of N = 8192 points, seeded
    assert (AG.B, AG.N) == (B, N)
    return [AG._batch(900 + 10 * i) for i in range(3)]


def _opt_state(model, opt):
    return ([x.detach().clone() for x in list(model.parameters()) + list(model.buffers())]
            + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.max_exp_avg_sq.clone(), opt.t.clone()], opt.steps)


def test_captured_step_with_flat_adam_equals_the_eager_loop(batches):
    """train.CapturedStep(model, FlatAdam, ..., after_backward=bucket.pack, defer_weight_grads=False) with its default warm-up: directly
    after construction the parameters, buffers, moments, amsgrad maximum, device counter t and host counter are what they were before
    it (fresh optimizer: zero moments, t = 0); three replays on three batches equal the same steps run eagerly by a second FlatAdam on a
    copy of the model.  Then the construction check again, with the eager twin's optimizer, which has stepped.
    defer_weight_grads=False: under Adam a reordered gradient sum is not comparable -- a noise-level gradient moves its parameter by
    +-lr in the first steps whatever its size."""
    import test_gpu_autograph as AG
    from crfconv_amd import models, optim
    from crfconv_amd.distributed import FlatGradAllReduce
    from crfconv_amd.train import CapturedStep
    cw = torch.linspace(0.5, 1.5, 13, device=DEV)

    def loss_fn(out, d):
        return F.cross_entropy(out, d.y.reshape(-1) - 1, weight=cw, ignore_index=-1)
    torch.manual_seed(5)
    ref = models.PointConvBig(6, 13, True, 3).to(DEV).train()
    net = models.PointConvBig(6, 13, True, 3).to(DEV).train()
    net.load_state_dict(ref.state_dict())
    rbucket, bucket = FlatGradAllReduce(ref), FlatGradAllReduce(net)
    mk = lambda b: optim.FlatAdam(b, lr=1e-3, weight_decay=1e-4, amsgrad=True)      # noqa: E731
    ropt, opt = mk(rbucket), mk(bucket)

    def eager_step(m, o, b, d):
        o.zero_grad()
        loss = loss_fn(m(d), d)
        loss.backward()
        b.pack()
        o.step()
        return float(loss)
    ref_losses = [eager_step(ref, ropt, rbucket, d) for d in batches]
    static = AG._batch(900)                                  # the resident batch the graph reads
    before, steps0 = _opt_state(net, opt)
    step = CapturedStep(net, opt, loss_fn, static, after_backward=bucket.pack, defer_weight_grads=False)
    after, steps1 = _opt_state(net, opt)
    assert all(torch.equal(a, b) for a, b in zip(after, before)) and steps1 == steps0 == 0
    assert int(opt.t) == 0 and float(opt.exp_avg.abs().max()) == 0.0 and float(opt.exp_avg_sq.abs().max()) == 0.0
    got_losses = [float(step(d)) for d in batches]
    torch.cuda.synchronize()
    assert int(opt.t) == 3
    for a, b in zip(got_losses, ref_losses):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (got_losses, ref_losses)
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert_close(a.float(), b.float(), 2e-5, 'after 3 steps: ' + k, tighten=False)
    # an optimizer that has stepped (the eager twin's: three eager steps, never captured): the warm-up of a construction must put back
    # exactly that state
    before, steps0 = _opt_state(ref, ropt)
    flat0 = ropt.flat.clone()
    assert int(ropt.t) == 3 and steps0 == 3 and float(ropt.max_exp_avg_sq.abs().max()) > 0
    rstep = CapturedStep(ref, ropt, loss_fn, static, after_backward=rbucket.pack, defer_weight_grads=False)
    after, steps1 = _opt_state(ref, ropt)
    assert all(torch.equal(a, b) for a, b in zip(after, before)) and steps1 == steps0
    rstep(batches[0])
    torch.cuda.synchronize()
    assert int(ropt.t) == 4 and bool(torch.isfinite(ropt.flat).all()) and not torch.equal(ropt.flat, flat0)


def test_captured_step_still_refuses_torch_adam_with_a_warm_up(batches):
    from crfconv_amd import models
    from crfconv_amd.train import CapturedStep
    net = models.PointConvBig(6, 13, True, 3).to(DEV).train()
    with pytest.raises(TypeError, match='FlatAdam'):
        CapturedStep(net, torch.optim.Adam(net.parameters()), lambda o, d: o.sum(), batches[0])


@pytest.fixture
def autograph_on():
    from crfconv_amd import train as tr
    was = tr._AUTO['on']
    tr.set_autograph(True)
    yield tr
    tr.set_autograph(was)


def test_flat_adam_after_a_captured_forward_recaptures_and_matches(autograph_on, batches):
    """The bare model with the self-capturing forward on (as test_p5_flat_sgd_after_capture_recaptures_and_matches): building a FlatAdam
    after a captured forward re-homes the parameters, the runner captures again -- once -- and two further steps match the eager twin:
    losses and gradients within that test's bounds.  Parameters: the runner's backward batches its weight-gradient sums, the eager
    twin's does not, so gradients differ in their last bits (GRAD_TOL), and where a gradient is at noise level Adam turns that into a
    difference of the order of lr whatever the gradient's size: |m^ / sqrt(v^)| <= 1 in step 1 and <= 1.01 in step 2 (Cauchy-Schwarz
    over the two gradients with betas (0.9, 0.999)), so one step moves an element by at most 1.01 lr and two trajectories part by at most
    2.02 lr per step.  Bound after step k: 2.02 k lr + PARAM_TOL, relative to max(1, |reference|) as everywhere (measured on MI355X with
    lr = 1e-3: 8.1e-5 after step 1, on conv4_1.lin_out.lin.weight).  A runner that went on replaying over the old parameter storage
    fails the capture count below and the loss of the second step."""
    import test_gpu_autograph as AG
    from crfconv_amd import distributed as D
    from crfconv_amd import optim
    lr = 1e-3
    net, ref = AG.twins()
    r = AG.warm_step(net, ref, AG.sgd(net), AG.sgd(ref), batches[0])
    captures = r.captures
    opts = []
    for m in (net, ref):
        bucket = D.FlatGradAllReduce(m)
        opts.append((bucket, optim.FlatAdam(bucket, lr=lr, weight_decay=1e-4)))
    for i, data in enumerate(batches[1:]):
        losses = []
        for m, (bucket, o) in zip((net, ref), opts):
            o.zero_grad()
            if m is net:
                loss = AG.crit(m(data), data)
                assert AG.graphed_passes(loss) == 1
                loss.backward()
            else:
                loss = AG.eager(lambda: AG.crit(m(data), data))
                loss.backward()
            bucket.pack()
            losses.append(loss.detach())
            del loss
        AG.same_loss(losses[0], losses[1], 'flat adam step %d' % i)
        AG.same_grads(net, ref, 'flat adam step %d' % i)
        for _, o in opts:
            o.step()
        pairs = []
        for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
            if a.is_floating_point():
                pairs.append((k, a.float(), b.float()))
            else:
                assert torch.equal(a, b), k
        AG.assert_all_close(pairs, 2.02 * (i + 1) * lr + AG.PARAM_TOL, 'flat adam step %d: parameters and buffers' % i, tighten=False)
    assert AG.runner_of(net) is r and r.captures == captures + 1, 'the re-homed parameters are captured anew, once'
    assert int(opts[0][1].t) == 2 and int(opts[1][1].t) == 2
