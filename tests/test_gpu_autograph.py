"""-m gpu: the self-capturing training forward (crfconv_amd.train: autograph, the product's default) against its autograph-off twin in
the caller patterns the reference loop does not use verbatim: two forwards under one loss, losses kept across a second forward, a stale
pass backpropagated again, parameters re-homed or re-assigned after the capture, hooks registered after it, logits kept across steps,
gradient accumulation, a skipped backward.  Every case starts two PointConvBig(6, 13, use_crf=True, steps=3) from equal state -- `net`
capturing itself, `ref` run launch by launch under train.no_autograph() -- drives both through the same pattern and compares losses,
kept logits, every .grad and the parameters / buffers after the optimizer step; it also asserts WHICH path ran (a _GraphedPass node in the
loss's graph, the runner's forward graph object the same as before), so that turning the capture off cannot pass for a fix.

B = 2 clouds of N = 8192 points: 16 384 rows, at least ops.state.mfma_min_rows, so the classifier runs the fused counter-keyed dropout --
equal BatchNorm step counters give both twins the same mask, and the oracle can be handed it (ops.dropout_keep_mask)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _seeded as S
from gpu_util import DEV, assert_close, assert_close_anchored, relerr, t
from oracle import crf_oracle as O

pytestmark = pytest.mark.gpu

B, N, T, NCLS = 2, 8192, 3, 13
# GRAD_TOL: the replayed backward batches its weight-gradient reductions (GraphedModel defer_weight_grads), the eager twin does not;
# the two orders differ by up to 1.7e-4 of a tensor's largest entry at some states (bit-identical replays whatever ran in between),
# the bound the oracle test of the replayed step states per tensor.  What these tests catch -- a backward over another pass's
# activations, a kept output overwritten, stale parameters -- is off by O(1).
LOSS_TOL, OUT_TOL, GRAD_TOL, PARAM_TOL = 1e-5, 2e-5, 5e-4, 2e-5


@pytest.fixture
def train():
    """autograph on for this test only (the suite's default is off: tests/conftest.py), the previous setting restored after it."""
    from crfconv_amd import train as tr
    was = tr._AUTO['on']
    tr.set_autograph(True)
    yield tr
    tr.set_autograph(was)


@pytest.fixture(autouse=True)
def _restore_host_threads():
    n = torch.get_num_threads()
    yield
    torch.set_num_threads(n)


def _batch(seed):
    import crfconv_amd
    pos = np.stack([S.make_cloud(seed + b, N, box=(2, 2, 1)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, N, 3), 0, 1)], -1)
    return crfconv_amd.multiscale_compute(t(pos), x=t(feats), y=t(S.integers(seed, 'y', (B, N), 0, 14)),
                                          generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope='module')
def batches():
    return [_batch(700 + 10 * i) for i in range(4)]


CW = None


def crit(out, data):
    """The reference's loss (trainval.py:101-104) with non-uniform class weights."""
    global CW
    if CW is None:
        CW = torch.linspace(0.5, 1.5, NCLS, device=DEV)
    return F.cross_entropy(out, data.y.reshape(-1) - 1, weight=CW, ignore_index=-1)


def twins(seed=6):
    from crfconv_amd import models
    torch.manual_seed(seed)
    ref = models.PointConvBig(6, NCLS, True, T).to(DEV).train()
    net = models.PointConvBig(6, NCLS, True, T).to(DEV).train()
    net.load_state_dict(ref.state_dict())
    return net, ref


def sgd(m):
    return torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.95, weight_decay=1e-4)


def graphed_passes(loss):
    """Number of replayed passes (_GraphedPass nodes) in the autograd graph behind `loss`."""
    seen, todo, n = {}, [loss.grad_fn], 0
    while todo:
        fn = todo.pop()
        if fn is None or id(fn) in seen:
            continue
        seen[id(fn)] = fn                               # (kept alive: an id is unique only while its object lives)
        if type(fn).__name__.startswith('_GraphedPass'):
            n += 1
            continue                                    # (its inputs are the parameters)
        todo.extend(f for f, _ in fn.next_functions)
    return n


def runner_of(net):
    r = net.__dict__.get('_autograph')
    assert r is not None and r.fwd_graph is not None and r.bwd_graph is not None, 'the model never captured itself'
    return r


def assert_all_close(pairs, tol, what, tighten=True):
    """assert_close over many tensors under ONE tolerance key: the worst of the per-tensor errors, each relative to max(1, |that
    tensor's reference|) -- as strict as one assert_close per tensor, without a baseline entry per tensor."""
    errs = [(relerr(a, b), k) for k, a, b in pairs]
    assert errs, what
    e, k = max(errs)
    try:
        assert_close(torch.tensor([e], dtype=torch.float64), torch.zeros(1, dtype=torch.float64), tol, what, tighten)
    except AssertionError as x:
        raise AssertionError('%s [worst tensor: %s]' % (x, k)) from None


def same_grads(net, ref, what):
    pairs = []
    for (k, a), b in zip(net.named_parameters(), ref.parameters()):
        assert (a.grad is None) == (b.grad is None), '%s: %s has a gradient on one side only' % (what, k)
        if b.grad is not None:
            pairs.append((k, a.grad, b.grad))
    assert_all_close(pairs, GRAD_TOL, what + ': every .grad')


def same_state(net, ref, what):
    """Parameters and buffers: floating ones within PARAM_TOL (a trajectory: tighten=False), step counters exactly."""
    assert '_autograph' not in ref.__dict__, 'the eager twin captured itself'
    pairs = []
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        if a.is_floating_point():
            pairs.append((k, a.float(), b.float()))
        else:
            assert torch.equal(a, b), '%s: %s differs' % (what, k)
    assert_all_close(pairs, PARAM_TOL, what + ': parameters and buffers', tighten=False)


def same_loss(a, b, what):
    assert_close(a.detach().reshape(1), b.detach().reshape(1), LOSS_TOL, what + ': loss')


def warm_step(net, ref, opt_n, opt_r, data):
    """One reference-loop step on both twins: `net` captures itself (capture + first replay); returns its runner."""
    from crfconv_amd import train as tr
    opt_n.zero_grad()
    loss = crit(net(data), data)
    assert graphed_passes(loss) == 1
    loss.backward()
    opt_n.step()
    opt_r.zero_grad()
    eager(lambda: crit(ref(data), data)).backward()
    opt_r.step()
    same_state(net, ref, 'after the warm step')
    return net if isinstance(net, tr.GraphedModel) else runner_of(net)


def eager(fn):
    from crfconv_amd import train as tr
    with tr.no_autograph():
        return fn()


# ------------------------------------------------------------------ P1: two forwards under one loss, outputs never named
def test_p1_two_forwards_one_loss_matches_eager_and_oracle(train, batches):
    from crfconv_amd import ops
    b0, b1, b2 = batches[:3]
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    bn = net.classifier[0].bn.batch_norm
    c0 = int(bn.num_batches_tracked)
    on.zero_grad(), orf.zero_grad()
    loss = crit(net(b1), b1) + crit(net(b2), b2)
    assert graphed_passes(loss) == 1, 'the first forward replays, the second runs eagerly (the first pass awaits its backward)'
    assert r.fwd_graph is fwd
    loss.backward()
    ref_loss = eager(lambda: crit(ref(b1), b1) + crit(ref(b2), b2))
    ref_loss.backward()
    same_loss(loss, ref_loss, 'P1')
    same_grads(net, ref, 'P1')
    assert int(bn.num_batches_tracked) == c0 + 2
    # the float64 oracle: the reference's loss of the two batches, each with the dropout mask its forward drew (counter c0 + 1, c0 + 2)
    seed = ops.dropout_seed(32, 128)
    masks = [torch.from_numpy(ops.dropout_keep_mask(seed, c0 + 1 + i, B * N * 128, 0.5).reshape(B, N, 128)).float() for i in range(2)]
    names = [k for k, p in net.named_parameters() if p.requires_grad]
    torch.set_num_threads(16)
    res = {}
    for tag, cast in (('f32', lambda v: v.clone()), ('f64', lambda v: v.double() if v.is_floating_point() else v.clone())):
        prm = {k: cast(v).requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
        total = 0
        for data, mask in zip((b1, b2), masks):
            ms = [{k: cast(getattr(l, k).cpu()) for k in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx') if getattr(l, k, None) is not None}
                  for l in data.multiscale]
            logits = O.pointconv_resnet(prm, cast(data.x.cpu()), ms, T, True, True, dropout_mask=cast(mask))
            total = total + O.training_loss(logits, data.y.cpu(), cast(CW.cpu()))
        total.backward()
        res[tag] = (total.detach(), {k: prm[k].grad.detach() for k in names})
        del prm
    (l32, g32), (l64, g64) = res['f32'], res['f64']
    assert_close_anchored(loss.detach().cpu(), l32, l64, 1e-5, 'P1 loss vs oracle')
    params = dict(net.named_parameters())
    for k in names:
        e, e32 = relerr(params[k].grad, g64[k]), relerr(g32[k], g64[k])
        assert e <= max(5e-4, 4.0 * e32), 'P1 %s: gradient err vs fp64 oracle %.2e (fp32 oracle %.2e)' % (k, e, e32)
    on.step(), orf.step()
    same_state(net, ref, 'P1 after step()')
    # the replays are back for the next step
    on.zero_grad()
    loss = crit(net(b0), b0)
    assert graphed_passes(loss) == 1 and r.fwd_graph is fwd
    loss.backward()


# ------------------------------------------------------------------ P2: two losses kept, then the two backward calls
@pytest.mark.parametrize('order', ['first_then_second', 'second_then_first'])
def test_p2_two_live_losses_backward_in_either_order(train, batches, order):
    b0, b1, b2 = batches[:3]
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    on.zero_grad(), orf.zero_grad()
    l1 = crit(net(b1), b1)
    l2 = crit(net(b2), b2)                      # l1 still reaches the first pass: this one must not replay over it
    assert graphed_passes(l1) == 1 and graphed_passes(l2) == 0 and r.fwd_graph is fwd
    k1, k2 = eager(lambda: crit(ref(b1), b1)), eager(lambda: crit(ref(b2), b2))
    for a, b in ((l1, k1), (l2, k2)) if order == 'first_then_second' else ((l2, k2), (l1, k1)):
        a.backward()
        b.backward()
    same_loss(l1, k1, 'P2 first')
    same_loss(l2, k2, 'P2 second')
    same_grads(net, ref, 'P2')
    on.step(), orf.step()
    same_state(net, ref, 'P2 after step()')
    on.zero_grad()
    loss = crit(net(b0), b0)
    assert graphed_passes(loss) == 1 and r.fwd_graph is fwd
    loss.backward()


# ------------------------------------------------------------------ P3: a stale pass backpropagated after a newer one replayed
def test_p3_stale_pass_backward_raises_on_the_bare_model(train, batches):
    b0, b1, b2, b3 = batches
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    on.zero_grad(), orf.zero_grad()
    l1 = crit(net(b1), b1)
    assert graphed_passes(l1) == 1
    l1.backward(retain_graph=True)
    k1 = eager(lambda: crit(ref(b1), b1))
    k1.backward(retain_graph=True)
    same_grads(net, ref, 'P3 first backward')
    for m, o, ev in ((net, on, False), (ref, orf, True)):      # a full step on b2
        o.zero_grad()
        loss = eager(lambda: crit(m(b2), b2)) if ev else crit(m(b2), b2)
        if not ev:
            assert graphed_passes(loss) == 1 and r.fwd_graph is fwd
        loss.backward()
        o.step()
    same_state(net, ref, 'P3 after the step on b2')
    # l1's activations were overwritten by b2's replay: its second backward must not run on them
    with pytest.raises(RuntimeError, match='saved activations are gone'):
        l1.backward()
    del l1, k1                                                 # (the eager twin cannot either: the step changed its weights in place)
    # the model goes on: the next step replays and matches
    for m, o in ((net, on), (ref, orf)):
        o.zero_grad()
    loss = crit(net(b3), b3)
    assert graphed_passes(loss) == 1 and r.fwd_graph is fwd
    loss.backward()
    k = eager(lambda: crit(ref(b3), b3))
    k.backward()
    same_loss(loss, k, 'P3 next step')
    same_grads(net, ref, 'P3 next step')


def test_p3_graphed_model_backward_over_a_newer_replay_raises(train, batches):
    """The explicit GraphedModel has no pending guard: the second forward of P1 replays over the first pass, whose backward must then
    raise rather than run on the second pass's activations."""
    b0, b1, b2, b3 = batches
    net, ref = twins()
    gm = train.GraphedModel(net)
    on, orf = sgd(gm), sgd(ref)
    warm_step(gm, ref, on, orf, b0)
    fwd = gm.fwd_graph
    on.zero_grad(), orf.zero_grad()
    loss = crit(gm(b1), b1) + crit(gm(b2), b2)
    assert graphed_passes(loss) == 2 and gm.fwd_graph is fwd
    with pytest.raises(RuntimeError, match='saved activations are gone'):
        loss.backward()
    del loss
    eager(lambda: crit(ref(b1), b1) + crit(ref(b2), b2))       # (the twin's dropout counters follow)
    for m, o in ((gm, on), (ref, orf)):
        o.zero_grad()
    loss = crit(gm(b3), b3)
    assert graphed_passes(loss) == 1 and gm.fwd_graph is fwd
    loss.backward()
    k = eager(lambda: crit(ref(b3), b3))
    k.backward()
    same_loss(loss, k, 'P3 GraphedModel next step')
    same_grads(gm.model, ref, 'P3 GraphedModel next step')
    on.step(), orf.step()
    same_state(gm.model, ref, 'P3 GraphedModel after step()')


# ------------------------------------------------------------------ P4: logits kept across steps
def test_p4_logits_kept_across_steps_keep_their_values(train, batches):
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    kept_n, kept_r, graphs = [], [], []
    for i, data in enumerate(batches[:3]):
        for m, o, keep in ((net, on, kept_n), (ref, orf, kept_r)):
            o.zero_grad()
            y_pred = m(data) if m is net else eager(lambda: m(data))
            keep.append(y_pred)
            loss = crit(y_pred, data)
            if m is net:
                assert graphed_passes(loss) == 1
                graphs.append(runner_of(net).fwd_graph)
            loss.backward()
            o.step()
        same_state(net, ref, 'P4 step %d' % i)
    assert graphs[0] is graphs[1] is graphs[2], 'one capture, three replays'
    for i, (a, b) in enumerate(zip(kept_n, kept_r)):
        assert_close(a, b, OUT_TOL, 'P4 logits of step %d, read after step 3' % i)
    assert not torch.equal(kept_n[0], kept_n[2])


# ------------------------------------------------------------------ P5: parameters re-homed / re-assigned after the capture
# A step releases its loss before the next forward, except where a test says otherwise: a live graph of an earlier pass holds the
# parameters' gradient accumulators, and the runner captures again only once none is left (it runs eagerly until then).
def test_p5_flat_sgd_after_capture_recaptures_and_matches(train, batches):
    from crfconv_amd import distributed as D
    from crfconv_amd import optim
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, batches[0])
    captures = getattr(r, 'captures', 0)
    opts = []
    for m in (net, ref):                                   # every parameter becomes a view of the flat vector (p.data = view)
        bucket = D.FlatGradAllReduce(m)
        opts.append((bucket, optim.FlatSGD(bucket, lr=1e-2, momentum=0.95, weight_decay=1e-4)))
    graphs = []
    for i, data in enumerate(batches[1:]):
        losses = []
        for m, (bucket, o) in zip((net, ref), opts):
            bucket.zero()
            loss = crit(m(data), data) if m is net else eager(lambda: crit(m(data), data))
            if m is net:
                assert graphed_passes(loss) == 1
                graphs.append(r.fwd_graph)
            loss.backward()
            bucket.pack()
            losses.append(loss.detach())
            del loss
        same_loss(losses[0], losses[1], 'P5 flat step %d' % i)
        same_grads(net, ref, 'P5 flat step %d' % i)
        for _, o in opts:
            o.step()
        same_state(net, ref, 'P5 flat step %d' % i)
    assert runner_of(net) is r and getattr(r, 'captures', 0) == captures + 1, 'the re-homed parameters are captured anew, once'
    assert graphs[0] is graphs[1] is graphs[2]


def test_p5_load_state_dict_assign_after_capture_recaptures_and_matches(train, batches):
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, batches[0])
    captures = getattr(r, 'captures', 0)
    on.zero_grad(), orf.zero_grad()
    live_n = crit(net(batches[0]), batches[0])             # a loss that stays alive across the move and the next call
    live_r = eager(lambda: crit(ref(batches[0]), batches[0]))
    live_n.backward(), live_r.backward()
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    for m in (net, ref):                                   # new Parameter / buffer objects at new addresses
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, assign=True)
    on, orf = sgd(net), sgd(ref)
    paths = []
    for i, data in enumerate(batches[1:]):
        on.zero_grad(), orf.zero_grad()
        ln = crit(net(data), data)
        paths.append((graphed_passes(ln), r.fwd_graph, getattr(r, 'captures', 0)))
        lr = eager(lambda: crit(ref(data), data))
        same_loss(ln, lr, 'P5 assign step %d' % i)
        ln.backward(), lr.backward()
        same_grads(net, ref, 'P5 assign step %d' % i)
        on.step(), orf.step()
        same_state(net, ref, 'P5 assign step %d' % i)
        del ln, lr
        if i == 0:
            del live_n, live_r
    assert runner_of(net) is r
    assert paths[0][0] == 0 and paths[0][1] is None, 'an earlier pass still alive: eagerly, no capture over its gradient accumulators'
    assert paths[1][0] == 1 and paths[1][2] == captures + 1, 'the earlier passes dropped: captured anew'
    assert paths[2][0] == 1 and paths[2][1] is paths[1][1] and paths[2][2] == captures + 1


# ------------------------------------------------------------------ P6: hooks registered after the capture
@pytest.mark.parametrize('kind', ['submodule', 'global'])
def test_p6_hooks_registered_after_capture_are_called(train, batches, kind):
    b0, b1, b2 = batches[:3]
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    seen = {'net': [], 'ref': []}
    mods = {id(m): 'net' for m in net.modules()}
    mods.update({id(m): 'ref' for m in ref.modules()})

    def hook(m, inp, out):
        side = mods.get(id(m))
        if side is not None and torch.is_tensor(out):
            seen[side].append((type(m).__name__, out.detach().clone()))
    if kind == 'submodule':
        handles = [net.conv1_1.register_forward_hook(hook), ref.conv1_1.register_forward_hook(hook)]
    else:
        handles = [torch.nn.modules.module.register_module_forward_hook(hook)]
    try:
        on.zero_grad(), orf.zero_grad()
        ln = crit(net(b1), b1)
        assert graphed_passes(ln) == 0, 'a hook registered since the capture: the model runs its own forward'
        lr = eager(lambda: crit(ref(b1), b1))
        ln.backward(), lr.backward()
    finally:
        for h in handles:
            h.remove()
    assert seen['net'] and len(seen['net']) == len(seen['ref'])
    assert [n for n, _ in seen['net']] == [n for n, _ in seen['ref']]
    assert_all_close([(n, a, b) for (n, a), (_, b) in zip(seen['net'], seen['ref'])], OUT_TOL, 'P6 hooked outputs')
    same_loss(ln, lr, 'P6')
    same_grads(net, ref, 'P6')
    on.step(), orf.step()
    same_state(net, ref, 'P6 after step()')
    # hooks removed: the replays are back, without a recapture
    on.zero_grad(), orf.zero_grad()
    ln = crit(net(b2), b2)
    assert graphed_passes(ln) == 1 and r.fwd_graph is fwd
    lr = eager(lambda: crit(ref(b2), b2))
    ln.backward(), lr.backward()
    same_loss(ln, lr, 'P6 after remove()')
    same_grads(net, ref, 'P6 after remove()')


# ------------------------------------------------------------------ P7: gradient accumulation over two micro-batches
def test_p7_gradient_accumulation_on_the_bare_model(train, batches):
    b0, b1, b2 = batches[:3]
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    for step in range(2):
        on.zero_grad(), orf.zero_grad()
        for i, data in enumerate((b1, b2) if step == 0 else (b2, b1)):
            ln = crit(net(data), data)
            assert graphed_passes(ln) == 1 and r.fwd_graph is fwd
            ln.backward()
            lr = eager(lambda: crit(ref(data), data))
            lr.backward()
            same_loss(ln, lr, 'P7 step %d micro-batch %d' % (step, i))
        same_grads(net, ref, 'P7 step %d accumulated' % step)
        on.step(), orf.step()
        same_state(net, ref, 'P7 step %d' % step)


# ------------------------------------------------------------------ P8: a skipped backward
def test_p8_skipped_backward_dropped_or_kept_loss(train, batches):
    b0, b1, b2, b3 = batches
    net, ref = twins()
    on, orf = sgd(net), sgd(ref)
    r = warm_step(net, ref, on, orf, b0)
    fwd = r.fwd_graph
    on.zero_grad(), orf.zero_grad()
    # the loss dropped without a backward (say, NaN): nothing reaches that pass any more, the next call replays
    ln = crit(net(b1), b1)
    del ln
    lr = eager(lambda: crit(ref(b1), b1))
    del lr
    ln = crit(net(b2), b2)
    assert graphed_passes(ln) == 1 and r.fwd_graph is fwd
    lr = eager(lambda: crit(ref(b2), b2))
    ln.backward(), lr.backward()
    same_loss(ln, lr, 'P8 dropped')
    same_grads(net, ref, 'P8 dropped')
    on.step(), orf.step()
    same_state(net, ref, 'P8 dropped, after step()')
    # the same line, the loss kept: the next call runs eagerly, and the kept pass can still be backpropagated correctly
    on.zero_grad(), orf.zero_grad()
    kn = crit(net(b1), b1)
    kr = eager(lambda: crit(ref(b1), b1))
    ln = crit(net(b3), b3)
    assert graphed_passes(kn) == 1 and graphed_passes(ln) == 0
    lr = eager(lambda: crit(ref(b3), b3))
    ln.backward(), lr.backward()
    same_loss(ln, lr, 'P8 kept, next call')
    same_grads(net, ref, 'P8 kept, next call')
    held = [(p.grad.clone(), q.grad.clone()) for p, q in zip(net.parameters(), ref.parameters())]
    on.zero_grad(), orf.zero_grad()
    kn.backward(), kr.backward()
    same_loss(kn, kr, 'P8 kept loss')
    same_grads(net, ref, 'P8 kept loss, backward after the next call')
    for (p, q), (gp, gq) in zip(zip(net.parameters(), ref.parameters()), held):
        p.grad += gp
        q.grad += gq
    on.step(), orf.step()
    same_state(net, ref, 'P8 kept, after step()')
    del kn, kr
    on.zero_grad()
    ln = crit(net(b0), b0)
    assert graphed_passes(ln) == 1 and r.fwd_graph is fwd
    ln.backward()
