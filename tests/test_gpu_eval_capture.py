"""The eval / no_grad forward that captures itself (train.GraphedInference, PointConvBig's own eval runner, train.stats) and the
classifier head of that forward as one launch (ops.head_eval, InferenceNet(fused_head=True), the NULL-mask form of
crfconv_head_forward).  Network tests run at B = 2, N = 4096, 13 classes, 3 mean-field steps, K = 16 -- the smallest cloud whose
fifth level (16 points) still holds 16 neighbours -- with weights and BatchNorm state from _seeded.fill_state_dict."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _seeded as S
from gpu_util import DEV, assert_close_anchored, t
from oracle import crf_oracle as O
from test_gpu_infer import B, N, NCLS, OUT_TOL, STEPS, count_calls, make_batch, make_net, min_rows, rows, seeded_mlp

pytestmark = pytest.mark.gpu

HEAD_SEED = 1234          # any value: at p = 0 the mask keeps every element


# ------------------------------------------------------------------------------------------------------------------ the head operator
def head_parts(M, Ci, C2, bias, seed):
    """(x, W1, coef [4, 128], slope, W2, b2) of a seeded classifier head on the device."""
    from crfconv_amd import ops
    mlp = seeded_mlp(Ci, 128, 0.1, seed)
    coef = ops.bn_eval_coefs([mlp.bn.batch_norm])[1][0]
    W2 = t(S.uniform(seed, 'W2', (C2, 128), -0.3, 0.3).astype(np.float32))
    b2 = t(S.uniform(seed, 'b2', (C2,), -0.5, 0.5).astype(np.float32)) if bias else None
    return rows(seed, 'x', M, Ci), mlp.lin.weight.detach(), coef, 0.1, W2, b2


def head_library_call(x, W1, coef, slope, W2, b2, p=0.0, with_mask=True, out=None):
    """crfconv_head_forward itself: with a mask buffer and a counter (the training form: at p = 0 the parent's kernel), or with
    NULL for mask, counter and counter_used (the eval form).  out: an over-allocated logits buffer to write into."""
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    m, ci = x.shape
    co, c2 = W1.shape[0], W2.shape[0]
    logits = torch.empty((m, c2), dtype=torch.float32, device=x.device) if out is None else out
    mask = counter = None
    if with_mask:
        mask = torch.zeros(_lib.load().crfconv_head_mask_words(m), dtype=torch.int32, device=x.device)
        counter = torch.full((1,), 5, dtype=torch.int64, device=x.device)
    _lib.call('crfconv_head_forward', ptr(x), ptr(W1), ptr(coef), float(slope), float(p), HEAD_SEED, ptr(counter), ptr(W2), ptr(b2),
              m, ci, co, c2, ptr(logits), ptr(mask), None, stream_ptr())
    return logits, mask


def head_formula(x, W1, coef, slope, W2, b2, dtype):
    """logits = lrelu(a (x W1^T) + b, slope) W2^T + b2 on the CPU in `dtype`."""
    x, W1, coef, W2 = (v.detach().cpu().to(dtype) for v in (x, W1, coef, W2))
    h = F.leaky_relu(coef[0] * (x @ W1.T) + coef[1], slope)
    out = h @ W2.T
    return out if b2 is None else out + b2.detach().cpu().to(dtype)


# (M, Ci, C2, bias): one row; a partial first group; exactly one group on the narrow operand (NCH = 1); a one-row tail group and one
# class; the full class tile; 65537 rows -- a sweep is 512 workgroups x 4 wavefronts x 16 rows = 32768 rows, so the first wavefront
# walks three groups, the third a one-row tail, with the two-ahead operand request past the end
HEAD_CASES = [(1, 32, 13, True), (15, 32, 13, True), (16, 16, 8, False), (17, 32, 1, True), (1000, 16, 16, True), (65537, 32, 13, True)]


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_head_eval_equals_the_training_form_at_p_0_and_the_formula(case):
    from crfconv_amd import ops
    M, Ci, C2, bias = case
    parts = head_parts(M, Ci, C2, bias, 2000 + M + Ci + C2)
    with count_calls() as names:
        got = ops.head_eval(*parts)
    assert dict(names) == {'crfconv_head_forward': 1}
    assert got.shape == (M, C2) and got.grad_fn is None and not got.requires_grad
    parent, mask = head_library_call(*parts, p=0.0, with_mask=True)
    assert bool((mask == -1).all())                                      # (the training form really ran: at p = 0 every bit is set)
    assert torch.equal(got, parent), 'max |diff| %g' % float((got - parent).abs().max())
    assert_close_anchored(got, head_formula(*parts, torch.float32), head_formula(*parts, torch.float64), OUT_TOL, 'head_eval logits')
    # rows beyond M of an over-allocated, pre-filled buffer stay as they were
    big = torch.full((M + 16, C2), -7.5, dtype=torch.float32, device=DEV)
    head_library_call(*parts, with_mask=False, out=big)
    assert torch.equal(big[:M], got) and bool((big[M:] == -7.5).all())


def test_head_eval_takes_leading_dimensions_and_ignores_requires_grad():
    from crfconv_amd import ops
    x, W1, coef, slope, W2, b2 = head_parts(2 * 40, 32, 13, True, 77)
    flat = ops.head_eval(x, W1, coef, slope, W2, b2)
    W1g = W1.clone().requires_grad_(True)
    shaped = ops.head_eval(x.reshape(2, 40, 32), W1g, coef, slope, W2, b2)
    assert shaped.shape == (2, 40, 13) and shaped.grad_fn is None and torch.equal(shaped.reshape(-1, 13), flat)


def test_head_refusals():
    from crfconv_amd import _lib, ops
    x, W1, coef, slope, W2, b2 = head_parts(64, 32, 13, True, 5)
    wide = seeded_mlp(64, 128, 0.1, 6)
    with pytest.raises(_lib.CrfConvError, match='crfconv_head_supported'):           # Ci = 64
        ops.head_eval(rows(6, 'x', 64, 64), wide.lin.weight, coef, slope, W2, b2)
    narrow = seeded_mlp(32, 64, 0.1, 7)
    with pytest.raises(_lib.CrfConvError, match='crfconv_head_supported'):           # Co = 64
        ops.head_eval(x, narrow.lin.weight, ops.bn_eval_coefs([narrow.bn.batch_norm])[1][0], slope, W2[:, :64].contiguous(), b2)
    W17 = t(S.uniform(8, 'W2', (17, 128), -0.3, 0.3).astype(np.float32))
    with pytest.raises(_lib.CrfConvError, match='crfconv_head_supported'):           # C2 = 17
        ops.head_eval(x, W1, coef, slope, W17, None)
    with pytest.raises(_lib.CrfConvError, match='float32'):
        ops.head_eval(x.double(), W1, coef, slope, W2, b2)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        ops.head_eval(x.cpu(), W1.cpu(), coef.cpu(), slope, W2.cpu(), b2.cpu())
    with pytest.raises(_lib.CrfConvError, match='hidden channels'):
        ops.head_eval(x, W1, coef, slope, W2[:, :64].contiguous(), b2)
    # the library itself: the eval form (NULL mask) has no dropout
    with pytest.raises(_lib.CrfConvError, match='mask_bits is NULL .* p != 0 needs a mask buffer'):
        head_library_call(x, W1, coef, slope, W2, b2, p=0.5, with_mask=False)


def test_head_eval_against_the_two_launch_form_bit_identity_is_reported():
    """Information, not a criterion: the fused head and linear_bn_act + ops.linear need not share a summation order."""
    from crfconv_amd import ops
    x, W1, coef, slope, W2, b2 = head_parts(B * N, 32, NCLS, True, 91)
    fused = ops.head_eval(x, W1, coef, slope, W2, b2)
    for rows_min in (1, None):
        with min_rows(rows_min), torch.no_grad():
            two = ops.linear(ops.linear_bn_act(x, W1, coef, slope=slope), W2, b2)
        print('head_eval vs linear_bn_act + linear, %s: bit-identical %s, max |diff| %.3e, max |logit| %.3e'
              % ('min_rows(1)' if rows_min else 'default state', bool(torch.equal(fused, two)), float((fused - two).abs().max()),
                 float(two.abs().max())))
        assert float((fused - two).abs().max()) <= OUT_TOL * max(1.0, float(two.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope='module')
def batches():
    return make_batch(60), make_batch(70)


@pytest.fixture(scope='module')
def crf_net():
    return make_net(True, 11)


@pytest.fixture
def autograph():
    from crfconv_amd import train
    was = train._AUTO['on']
    train.set_autograph(True)
    try:
        yield train
    finally:
        train.set_autograph(was)


def eager_eval(net, batch):
    from crfconv_amd import train
    with train.no_autograph(), torch.no_grad():
        return net(batch)


def fresh_net(crf_net):
    """A copy of the module's network (no runner travels with a copy), in eval mode."""
    return copy.deepcopy(crf_net[0]).eval()


def batch_of(seed, n, ratios, labels=False):
    """make_batch at another size / with labels (the same subsets for every seed: load_ needs equal shapes)."""
    import crfconv_amd
    pos = np.stack([S.make_cloud(seed + b, n, box=(2.0, 2.0, 1.0)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, n, 3), 0, 1)], -1).astype(np.float32)
    choices, m = [], n
    for i, r in enumerate(ratios):
        choices.append(torch.from_numpy(S.permutation(40, 'c%d' % i, m)[: m // r]))
        m //= r
    y = t(S.integers(seed, 'y', (B, n), 0, NCLS + 1)) if labels else None
    return crfconv_amd.multiscale_compute(t(pos), x=t(feats), y=y, choices=choices, kernel_size=(16,) * 5)


def test_fused_head_network_against_the_oracle_and_its_calls(batches, crf_net):
    from crfconv_amd import InferenceNet
    net, sd = crf_net
    batch = batches[0]
    plain, fused = InferenceNet(net), InferenceNet(net, fused_head=True)
    with torch.no_grad():
        plain(batch), fused(batch)                         # (lazily built tables, the coefficient buffers)
        with count_calls() as base:
            ref_logits = plain(batch)
        with count_calls() as names:
            logits = fused(batch)
    assert logits.shape == (B * N, NCLS) and logits.grad_fn is None
    assert base['crfconv_head_forward'] == 0
    assert names['crfconv_head_forward'] == 1
    assert names['crfconv_linear_bn_act'] + names['crfconv_gemm_bn_act'] == 49
    assert base['crfconv_linear_bn_act'] + base['crfconv_gemm_bn_act'] == 50
    assert names['crfconv_linear_forward'] + names['crfconv_gemm'] == base['crfconv_linear_forward'] + base['crfconv_gemm'] - 1
    others = ('crfconv_head_forward', 'crfconv_linear_bn_act', 'crfconv_gemm_bn_act', 'crfconv_linear_forward', 'crfconv_gemm')
    assert {k: v for k, v in base.items() if k not in others} == {k: v for k, v in names.items() if k not in others}
    print('fused head vs default wrapper at the network level: bit-identical %s, max |diff| %.3e'
          % (bool(torch.equal(logits, ref_logits)), float((logits - ref_logits).abs().max())))
    ms = [{k: getattr(l, k).cpu() for k in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx') if getattr(l, k, None) is not None}
          for l in batch.multiscale]
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.pointconv_resnet({k: v.clone() for k, v in sd.items()}, batch.x.cpu(), ms, STEPS, False, True)
        ms64 = [{k: (v.double() if v.is_floating_point() else v) for k, v in l.items()} for l in ms]
        ref64 = O.pointconv_resnet({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()},
                                   batch.x.cpu().double(), ms64, STEPS, False, True)
    assert_close_anchored(logits, ref, ref64, OUT_TOL, 'InferenceNet(fused_head=True) logits')


def test_fused_head_outside_the_kernels_range_runs_the_two_launches(batches):
    """19 classes: more than the head kernel's class tile -- silently today's two launches, bit for bit."""
    from crfconv_amd import InferenceNet, models
    net = models.PointConvBig(6, 19, use_crf=True, steps=STEPS)
    net.load_state_dict(S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 15))
    net = net.to(DEV).eval()
    with torch.no_grad():
        ref = InferenceNet(net)(batches[0])
        with count_calls() as names:
            got = InferenceNet(net, fused_head=True)(batches[0])
    assert names['crfconv_head_forward'] == 0 and names['crfconv_linear_bn_act'] + names['crfconv_gemm_bn_act'] == 50
    assert got.shape == (B * N, 19) and torch.equal(got, ref)


REPLAYED_AWAY = ('crfconv_linear_bn_act', 'crfconv_gemm_bn_act', 'crfconv_pointconv_forward')


def test_the_bare_model_captures_its_eval_forward_and_replays(batches, crf_net, autograph):
    train = autograph
    net = fresh_net(crf_net)
    assert train.stats(net)['eval']['captures'] == 0
    ref0, ref1 = eager_eval(net, batches[0]), eager_eval(net, batches[1])
    assert '_autograph_eval' not in net.__dict__ and not torch.equal(ref0, ref1)
    with torch.no_grad():
        out0 = net(batches[0])
        st = train.stats(net)['eval']
        assert st['captures'] == 1 and sum(st['eager'].values()) == 0
        keep = out0.clone()
        with count_calls() as names:
            out1 = net(batches[1])
    st = train.stats(net)['eval']
    assert st['captures'] == 1 and st['replays'] == 2 and sum(st['eager'].values()) == 0
    assert out0.grad_fn is None and out0.shape == (B * N, NCLS)
    assert torch.equal(out0, ref0) and torch.equal(out1, ref1)
    assert torch.equal(out0, keep)                         # the first result is the caller's own: the second call left it alone
    for name in REPLAYED_AWAY:
        assert names[name] == 0, name
    assert not any(k.startswith('crfconv_meanfield_forward') for k in names), dict(names)
    assert list(net.state_dict()) == list(crf_net[0].state_dict())       # the runner is not part of the model's tree
    assert train.stats(net)['train'] == {'captures': 0, 'replays': 0, 'eager': {}}


def test_replays_read_the_live_state_and_rehomed_parameters_capture_again(batches, crf_net, autograph):
    train = autograph
    net = fresh_net(crf_net)
    batch = batches[0]
    with torch.no_grad():
        before = net(batch)
        net.conv1_1.lin_in.bn.batch_norm.running_var.mul_(1.7).add_(0.05)
        changed = net(batch)
        assert torch.equal(changed, eager_eval(net, batch)) and not torch.equal(changed, before)
        other = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 13)
        net.load_state_dict(other)                         # in place: the same storage
        loaded = net(batch)
        assert torch.equal(loaded, eager_eval(net, batch)) and not torch.equal(loaded, changed)
        assert train.stats(net)['eval']['captures'] == 1 and train.stats(net)['eval']['replays'] == 3
        p = net.deconv1.fusion_nn.lin.weight
        p.data = p.data.clone()                            # another address: the graph would read stale storage
        p.data.mul_(1.25)
        again = net(batch)
        st = train.stats(net)['eval']
        assert st['captures'] == 2 and sum(st['eager'].values()) == 0
        assert torch.equal(again, eager_eval(net, batch)) and not torch.equal(again, loaded)


def test_what_stays_eager_is_counted_by_reason(batches, crf_net, autograph):
    train = autograph
    net = fresh_net(crf_net)
    twin = fresh_net(crf_net)
    batch = batches[0]
    with torch.no_grad():
        first = net(batch)
    base = train.stats(net)['eval']
    assert base['captures'] == 1 and base['replays'] == 1

    def counted(why, n=1):
        st = train.stats(net)['eval']
        assert st['replays'] == base['replays'] and st['captures'] == 1, (why, st)
        assert st['eager'][why] == n and sum(st['eager'].values()) == sum(base['eager'].values()) + 1, (why, st)
        base['eager'] = st['eager']

    # eval with grad enabled: a differentiable output
    out = net(batch)
    assert out.requires_grad and out.grad_fn is not None and torch.equal(out.detach(), first)
    counted('grad')
    # another shape: 2048 points (five levels 2048 .. 16)
    small = batch_of(80, 2048, (2, 4, 4, 4, 2))
    with torch.no_grad():
        out = net(small)
    assert out.shape == (B * 2048, NCLS) and torch.equal(out, eager_eval(twin, small))
    counted('shape')
    # a forward hook: the model's own forward runs, and fires it
    fired = []
    handle = net.conv1_1.lin_in.register_forward_hook(lambda mod, inp, o: fired.append(tuple(o.shape)))
    try:
        with torch.no_grad():
            out = net(batch)
    finally:
        handle.remove()
    assert len(fired) == 1 and torch.equal(out, first)
    counted('hooks')
    # inside the caller's own capture: issued inline, no nested capture; the caller's graph replays correctly
    static = batch._apply(torch.clone)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad(), train.no_autograph():
        net(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = net(static)
    counted('capturing')
    static.load_(batches[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager_eval(twin, batches[1]))
    # switched off
    train.set_autograph(False)
    with torch.no_grad():
        out = net(batch)
    train.set_autograph(True)
    assert torch.equal(out, first)
    counted('off')
    # ... and the replays are still there
    with torch.no_grad():
        assert torch.equal(net(batches[1]), eager_eval(twin, batches[1]))
    st = train.stats(net)['eval']
    assert st['replays'] == base['replays'] + 1 and st['captures'] == 1

    # no_grad in training mode: BatchNorm statistics advance, as today
    net.train(), twin.train()
    twin.load_state_dict(net.state_dict())
    tracked = int(net.conv1_1.lin_in.bn.batch_norm.num_batches_tracked)
    with torch.no_grad():
        torch.manual_seed(123)                             # (the classifier's dropout takes its seed from torch's generator)
        out = net(batch)
        torch.manual_seed(123)
        with train.no_autograph():
            ref = twin(batch)
    assert int(net.conv1_1.lin_in.bn.batch_norm.num_batches_tracked) == tracked + 1
    assert torch.equal(out, ref)
    for (k, a), b in zip(net.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b), k
    base['replays'] += 1
    counted('training')
    # (that first training forward made the step counters views of one vector: other buffer objects, so the next eval call captures again)
    net.load_state_dict(crf_net[1]), twin.load_state_dict(crf_net[1])
    net.eval(), twin.eval()
    with torch.no_grad():
        assert torch.equal(net(batch), first)
    assert train.stats(net)['eval']['captures'] == 2


def test_hooks_on_the_model_itself_fire_once_and_other_networks_stay_eager(batches, crf_net, autograph):
    """The model's own runner hands a call it cannot replay back to the model's forward -- no nested model(batch): a forward hook
    and a pre-hook on the ROOT module fire once per call, before the first capture and after it.  A subclass with its own _forward,
    a model with mixed decoders and a model with a phase_hook are not the network the runner replays: they run their own forward."""
    from crfconv_amd import models
    train = autograph
    batch = batches[0]
    ref = eager_eval(crf_net[0], batch)
    for capture_first in (False, True):
        net = fresh_net(crf_net)
        if capture_first:
            with torch.no_grad():
                net(batch)
            assert train.stats(net)['eval']['captures'] == 1
        fired = []
        h1 = net.register_forward_hook(lambda mod, inp, out: (fired.append('post'), out + 1.0)[1])
        h2 = net.register_forward_pre_hook(lambda mod, inp: fired.append('pre'))
        try:
            with torch.no_grad():
                out = net(batch)
        finally:
            h1.remove(), h2.remove()
        assert fired == ['pre', 'post'], fired
        assert torch.equal(out, ref + 1.0)                  # the hook's change of the output, applied once
        st = train.stats(net)['eval']
        assert st['eager'] == ({'hooks': 1} if capture_first else {}) and st['replays'] == (1 if capture_first else 0)
        assert ('_autograph_eval' in net.__dict__) is capture_first      # a hooked model creates no runner, as in training mode
    # calls that are switched off or bypassed in training mode are not counted as eval fallbacks
    net = fresh_net(crf_net)
    with torch.no_grad():
        net(batch)
        net.train()
        with train.no_autograph():
            net(batch)
        train.set_autograph(False)
        net(batch)
        train.set_autograph(True)
    assert sum(train.stats(net)['eval']['eager'].values()) == 0
    net.load_state_dict(crf_net[1])
    net.eval()

    class Doubled(models.PointConvBig):
        def _forward(self, data):
            return 2.0 * super()._forward(data)
    sub = Doubled(6, NCLS, use_crf=True, steps=STEPS)
    sub.load_state_dict(crf_net[1])
    sub = sub.to(DEV).eval()
    mixed = fresh_net(crf_net)
    mixed.deconv2 = models.point_conv_big.Upsampling(128, 64, 64).to(DEV).eval()
    hooked = fresh_net(crf_net)
    phases = []
    hooked.phase_hook = phases.append
    with torch.no_grad():
        assert torch.equal(sub(batch), 2.0 * ref) and '_autograph_eval' not in sub.__dict__
        assert torch.equal(mixed(batch), eager_eval(mixed, batch)) and '_autograph_eval' not in mixed.__dict__
        assert torch.equal(hooked(batch), ref) and torch.equal(hooked(batch), ref)
    assert phases == ['coarse', 'coarse'] and train.stats(hooked)['eval']['eager'] == {'phase': 2}


def test_training_and_eval_runners_alternate_on_one_model(crf_net, autograph):
    """The reference epoch in miniature: two training steps, one validation call, two more steps, one more call -- on the bare model."""
    train = autograph
    net = fresh_net(crf_net).train()
    twin = fresh_net(crf_net)
    data = [batch_of(100 + 10 * i, N, (4, 4, 4, 4, 2), labels=True) for i in range(3)]
    cw = torch.linspace(0.5, 1.5, NCLS, device=DEV)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)

    def train_step(d):
        opt.zero_grad()
        y_pred = net(d)
        assert type(y_pred.grad_fn).__name__.startswith('_GraphedPass'), type(y_pred.grad_fn).__name__
        loss = F.cross_entropy(y_pred, d.y.reshape(-1) - 1, weight=cw, ignore_index=-1)
        loss.backward()
        opt.step()

    def validate(d):
        net.eval()
        with torch.no_grad():
            out = net(d)
        net.train()
        twin.load_state_dict(net.state_dict())
        assert torch.equal(out, eager_eval(twin, d))
        return out
    train_step(data[0]), train_step(data[1])
    v1 = validate(data[2])
    train_step(data[0]), train_step(data[1])
    v2 = validate(data[2])
    assert not torch.equal(v1, v2) and bool(torch.isfinite(v2).all())
    st = train.stats(net)
    # (the training steps came first: the step counters were re-homed before the first validation call, so ONE eval capture serves both)
    assert st['eval']['captures'] == 1 and st['eval']['replays'] == 2 and sum(st['eval']['eager'].values()) == 0
    assert st['train']['captures'] == 1 and st['train']['replays'] == 4 and sum(st['train']['eager'].values()) == 0


def test_explicit_runner_with_a_fused_head_and_runners_do_not_travel(batches, crf_net, autograph):
    from crfconv_amd import InferenceNet
    train = autograph
    net = fresh_net(crf_net)
    fast = InferenceNet(net, fused_head=True)
    runner = train.GraphedInference(fast)
    with torch.no_grad():
        refs = [fast(b) for b in batches]
        with count_calls() as names:
            outs = [runner(b) for b in batches]
    assert torch.equal(outs[0], refs[0]) and torch.equal(outs[1], refs[1]) and not torch.equal(outs[0], outs[1])
    st = train.stats(runner)['eval']
    assert st['captures'] == 1 and st['replays'] == 2 and sum(st['eager'].values()) == 0
    assert '_autograph_eval' not in net.__dict__           # the explicit runner is the caller's, not the model's
    # the model's own runner: a copy starts without it, to() drops it
    with torch.no_grad():
        net(batches[0])
    assert net.__dict__.get('_autograph_eval') is not None
    assert '_autograph_eval' not in copy.deepcopy(net).__dict__
    net.to(DEV)
    assert '_autograph_eval' not in net.__dict__
    assert train.stats(net)['eval']['captures'] == 0
