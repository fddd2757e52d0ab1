"""InferenceNet and ops.linear_bn_act: the eval-mode MLP blocks as one launch each, bit for bit against today's eval path
(ops.linear -> ops.bn_act(eval) -> ops.add_lrelu, net.eval()(data)) and against the CPU oracle.  Every BatchNorm gets non-trivial
running statistics and affine parameters from _seeded.fill_state_dict: a fresh module's mean 0 / variance 1 would hide a wrong
coefficient row."""
import collections

import numpy as np
import pytest
import torch
import torch.nn as nn

import _seeded as S
from gpu_util import DEV, assert_close_anchored, t
from oracle import crf_oracle as O

pytestmark = pytest.mark.gpu

# tests/test_gpu_model.py: OUT_TOL = 1e-4 ("per-point logits within 1e-4", BASELINE.json north_star), applied as _eval_net_vs_oracle
# applies it: anchored on the float64 oracle, normalised by max(1, |ref|)
OUT_TOL = 1e-4


def seeded_mlp(ci, co, slope, seed, bias=False):
    from crfconv_amd.models.common import MLP
    mlp = MLP(ci, co, activation=None if slope == 1.0 else nn.LeakyReLU(negative_slope=slope))
    if bias:
        mlp.lin = nn.Linear(ci, co, bias=True)
    mlp.load_state_dict(S.fill_state_dict({k: tuple(v.shape) for k, v in mlp.state_dict().items()}, seed))
    return mlp.to(DEV).eval()


def rows(seed, name, m, c):
    return t(S.uniform(seed, name, (m, c), -1.0, 1.0).astype(np.float32))


class min_rows:
    """ops.state.mfma_min_rows = n inside the block (None: the default state)."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from crfconv_amd import ops
        self.prev = ops.state.mfma_min_rows
        if self.n is not None:
            ops.state.mfma_min_rows = self.n

    def __exit__(self, *exc):
        from crfconv_amd import ops
        ops.state.mfma_min_rows = self.prev
        return False


class count_calls:
    """Counts crfconv_amd._lib.call by entry-point name inside the block."""

    def __enter__(self):
        from crfconv_amd import _lib
        self.lib, self.orig, self.names = _lib, _lib.call, collections.Counter()

        def counting(name, *args):
            self.names[name] += 1
            return self.orig(name, *args)
        _lib.call = counting
        return self.names

    def __exit__(self, *exc):
        self.lib.call = self.orig
        return False


# ------------------------------------------------------------------------------------------------------------------ the operator
# (M, Ci, Co, slope, skip, split of the two-pointer operand or None)
STREAMING = [
    (1000, 6, 8, 0.1, False, None),          # element-wise path, row tail
    (1000, 6, 32, 1.0, False, None),         # shortcut: no activation
    (1000, 8, 32, 0.01, True, None),         # join
    (777, 32, 128, 0.1, False, None),        # two column slabs
    (520, 256, 64, 0.1, False, None),        # rolled chunk loop, reduced TCO
    (1000, 64, 32, 0.1, False, 32),          # two-pointer operand
    (40, 16, 8, 0.1, False, None),           # fewer rows than one workgroup
]
TILED = [
    (100, 512, 512, 0.01, True, None),       # join on the tiled kernel
    (640, 512, 256, 0.1, False, None),       # activation only
    (33, 6, 8, 0.1, False, None),            # small, unaligned K
    (160, 128, 512, 0.01, True, None),       # join, wide output
    (640, 64, 32, 0.1, False, 32),           # cat2 in front of the tiled kernel
]


def _operator_case(case, streaming):
    from crfconv_amd import ops
    M, Ci, Co, slope, with_skip, split = case
    seed = 1000 + M + Ci + Co
    # a join is a BatchNorm without activation followed by add + LeakyReLU(slope)
    mlp = seeded_mlp(Ci, Co, 1.0 if with_skip else slope, seed)
    W, bn = mlp.lin.weight, mlp.bn.batch_norm
    x = rows(seed, 'x', M, Ci)
    skip = rows(seed, 'skip', M, Co) if with_skip else None
    xa, xb = (x[:, :split].contiguous(), x[:, split:].contiguous()) if split else (x, None)
    with min_rows(1 if streaming else None), torch.no_grad():
        assert ops._mfma_ok(M, Ci, Co) is streaming          # the case runs the kernel it is listed under
        # today's sequence
        xin = ops.cat2(xa, xb) if split else x
        ref = ops.bn_act(ops.linear(xin, W), bn, False, 1.0 if with_skip else slope)
        if with_skip:
            ref = ops.add_lrelu(ref, skip, slope)
        _, (coef,) = ops.bn_eval_coefs([bn])
        with count_calls() as names:
            got = ops.linear_bn_act(xa, W, coef, slope=slope, skip=skip, xb=xb)
    assert got.grad_fn is None and not got.requires_grad
    assert got.shape == ref.shape and torch.equal(got, ref), 'max |diff| %g' % float((got - ref).abs().max())
    want = {'crfconv_linear_bn_act': 1} if streaming else {'crfconv_gemm_bn_act': 1}
    if split and not streaming:
        want['crfconv_cat2'] = 1
    assert dict(names) == want


@pytest.mark.parametrize('case', STREAMING, ids=lambda c: 'x'.join(str(v) for v in c[:3]))
def test_linear_bn_act_row_streaming_kernel_bit_for_bit(case):
    _operator_case(case, True)


@pytest.mark.parametrize('case', TILED, ids=lambda c: 'x'.join(str(v) for v in c[:3]))
def test_linear_bn_act_tiled_kernel_bit_for_bit(case):
    _operator_case(case, False)


def test_linear_bn_act_with_a_bias_in_front_of_the_batchnorm():
    """The optional bias goes into the accumulator as the product kernels add it, in front of the BatchNorm."""
    from crfconv_amd import ops
    for streaming in (True, False):
        mlp = seeded_mlp(16, 32, 0.1, 77, bias=True)
        x = rows(77, 'x', 300, 16)
        with min_rows(1 if streaming else None), torch.no_grad():
            ref = ops.bn_act(ops.linear(x, mlp.lin.weight, mlp.lin.bias), mlp.bn.batch_norm, False, 0.1)
            got = ops.linear_bn_act(x, mlp.lin.weight, ops.bn_eval_coefs([mlp.bn.batch_norm])[1][0], slope=0.1, bias=mlp.lin.bias)
        assert torch.equal(got, ref)


def test_bn_eval_coefs_equal_the_eval_branch_of_bn_forward():
    """One launch for many BatchNorms (more than one job table's 64) writes the rows crfconv_bn_forward(use_batch_stats=0) writes."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    widths = [4, 8, 32, 128, 260, 512, 1024] + [8] * 60
    bns = [seeded_mlp(4, C, 1.0, 300 + i).bn.batch_norm for i, C in enumerate(widths)]
    with count_calls() as names:
        flat, views = ops.bn_eval_coefs(bns)
    assert dict(names) == {'crfconv_bn_eval_coef_jobs': 1}
    assert flat.numel() == 4 * sum(widths) and len(views) == len(bns)
    for bn, view in zip(bns, views):
        C = bn.num_features
        x = torch.zeros((8, C), device=DEV)
        coef = torch.empty(4 * C, device=DEV)
        nbytes = _lib.load().crfconv_bn_workspace(8, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call('crfconv_bn_forward', ptr(x), 8, C, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), 0.1,
                  float(bn.eps), 0, 1.0, ptr(coef), ptr(torch.empty_like(x)), ptr(ws), nbytes, stream_ptr())
        assert view.shape == (4, C) and torch.equal(view.reshape(-1), coef), C
        assert float((view[0] - 1.0).abs().min()) > 0 and float(view[1].abs().max()) > 0      # a non-trivial state


def test_linear_bn_act_refusals():
    from crfconv_amd import _lib, ops
    mlp = seeded_mlp(16, 32, 0.1, 5)
    coef = ops.bn_eval_coefs([mlp.bn.batch_norm])[1][0]
    x = rows(5, 'x', 64, 16)
    with pytest.raises(_lib.CrfConvError, match='float32'):
        ops.linear_bn_act(x.double(), mlp.lin.weight, coef)
    with pytest.raises(Exception):
        ops.linear_bn_act(x.cpu(), mlp.lin.weight.cpu(), coef.cpu())
    with pytest.raises(_lib.CrfConvError, match='multiple of 4'):
        ops.linear_bn_act(x, mlp.lin.weight[:30].contiguous(), coef[:, :30].contiguous())


# ------------------------------------------------------------------------------------------------------------------ the network
B, N, STEPS, NCLS = 2, 4096, 3, 13


def make_batch(seed):
    import crfconv_amd
    pos = np.stack([S.make_cloud(seed + b, N, box=(2.0, 2.0, 1.0)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, N, 3), 0, 1)], -1).astype(np.float32)
    choices, n = [], N
    for i, r in enumerate((4, 4, 4, 4, 2)):
        choices.append(torch.from_numpy(S.permutation(40, 'c%d' % i, n)[: n // r]))       # one subset for every batch: load_ needs equal shapes
        n //= r
    return crfconv_amd.multiscale_compute(t(pos), x=t(feats), choices=choices, kernel_size=(16,) * 5)


def make_net(use_crf, seed):
    from crfconv_amd import models
    net = models.PointConvBig(6, NCLS, use_crf=use_crf, steps=STEPS)
    sd = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)      # random-gain weights, non-trivial BatchNorm state
    net.load_state_dict(sd)
    return net.to(DEV).eval(), sd


@pytest.fixture(scope='module')
def batch():
    return make_batch(60)


@pytest.fixture(scope='module')
def crf_net():
    return make_net(True, 11)


def n_bn_mlps(net):
    from crfconv_amd.models.common import MLP
    return sum(1 for name, m in net.named_modules() if isinstance(m, MLP) and m.bn is not None and 'weight_nn' not in name)


@pytest.mark.parametrize('use_crf', [True, False], ids=['crf', 'upsampling'])
def test_whole_network_bit_for_bit(batch, crf_net, use_crf):
    """InferenceNet(net)(data) == net.eval()(data): with every layer on the tiled kernel (the default state at 8192 rows), with levels 0
    and 1 on the row-streaming kernel, and again after load_state_dict of other weights without rebuilding the wrapper."""
    from crfconv_amd import InferenceNet
    net = crf_net[0] if use_crf else make_net(False, 12)[0]
    fast = InferenceNet(net).eval()
    try:
        for rows_min in (None, 1024):
            with min_rows(rows_min), torch.no_grad():
                ref = net(batch)
                got = fast(batch)
            assert got.shape == (B * N, NCLS) and got.grad_fn is None and bool(torch.isfinite(got).all())
            assert torch.equal(got, ref), (rows_min, float((got - ref).abs().max()))
        other = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 13)
        net.load_state_dict(other)
        with torch.no_grad():
            ref2, got2 = net(batch), fast(batch)
        assert not torch.equal(ref2, ref) and torch.equal(got2, ref2)
    finally:
        if use_crf:
            net.load_state_dict(crf_net[1])                # the module-scoped network goes back to its own weights


def test_whole_network_against_the_oracle(batch, crf_net):
    """The same small batch against oracle.crf_oracle.pointconv_resnet in float32 and float64, directly."""
    from crfconv_amd import InferenceNet
    net, sd = crf_net
    with torch.no_grad():
        logits = InferenceNet(net)(batch)
    ms = [{k: getattr(l, k).cpu() for k in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx') if getattr(l, k, None) is not None}
          for l in batch.multiscale]
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.pointconv_resnet({k: v.clone() for k, v in sd.items()}, batch.x.cpu(), ms, STEPS, False, True)
        ms64 = [{k: (v.double() if v.is_floating_point() else v) for k, v in l.items()} for l in ms]
        ref64 = O.pointconv_resnet({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()},
                                   batch.x.cpu().double(), ms64, STEPS, False, True)
    assert_close_anchored(logits, ref, ref64, OUT_TOL, 'InferenceNet logits')


# launches behind one library call, where that is not one: crfconv_bn_forward in eval mode on these row counts is the coefficient
# launch and the apply launch (csrc/bn.hip, crfconv_bn_forward: bn_coef_eval_kernel, bn_apply_kernel)
LAUNCHES = {'crfconv_bn_forward': 2}


def test_the_fused_path_really_ran(batch, crf_net):
    """Library calls of one forward, by name.  No stand-alone BatchNorm or join call is left; the one-launch blocks are as many as the
    BatchNorm-carrying MLPs outside weight_nn (50); one coefficient call.  Today's eval path spends three LAUNCHES on each of those
    MLPs (product, coefficients, apply) in two library CALLS (crfconv_bn_forward issues two of the launches), so the saving of "at
    least twice the MLP count" is a statement about launches: it is asserted on the launches behind the counted calls (LAUNCHES).
    Figures at B = 2, N = 4096, CRF decoders: the call counts and both differences are printed."""
    from crfconv_amd import InferenceNet
    net = crf_net[0]
    fast = InferenceNet(net)
    n = n_bn_mlps(net)
    assert n == 50 == len(fast.mlp_plan())
    with torch.no_grad():
        fast(batch)                                        # (lazily built tables, the coefficient buffer)
        with count_calls() as eager:
            net(batch)
        with count_calls() as fused:
            fast(batch)
    for name in ('crfconv_bn_forward', 'crfconv_bn_apply', 'crfconv_bn_apply_add', 'crfconv_add_lrelu'):
        assert fused[name] == 0, name
    assert fused['crfconv_linear_bn_act'] + fused['crfconv_gemm_bn_act'] == n
    assert 1 <= fused['crfconv_bn_eval_coef_jobs'] <= 2
    launches = lambda names: sum(k * LAUNCHES.get(name, 1) for name, k in names.items())
    print('library calls: eval %d, InferenceNet %d (difference %d); launches behind them: eval %d, InferenceNet %d (difference %d)'
          % (sum(eager.values()), sum(fused.values()), sum(eager.values()) - sum(fused.values()), launches(eager), launches(fused),
             launches(eager) - launches(fused)))
    assert sum(fused.values()) < sum(eager.values())
    assert launches(eager) - launches(fused) >= 2 * n
    # nothing but the MLP blocks changed: every other entry point is called as often as today
    mlp_names = {'crfconv_linear_forward', 'crfconv_gemm', 'crfconv_bn_forward', 'crfconv_add_lrelu', 'crfconv_cat2',
                 'crfconv_linear_bn_act', 'crfconv_gemm_bn_act', 'crfconv_bn_eval_coef_jobs'}
    assert {k: v for k, v in eager.items() if k not in mlp_names} == {k: v for k, v in fused.items() if k not in mlp_names}


def test_capturable_and_replays_follow_the_live_state(batch, crf_net):
    """The forward inside a caller's torch.cuda.graph (side-stream warm-up as SceneVoter._first): a replay on a second batch loaded
    into the static one, and a replay after an in-place change of a BatchNorm's running_var, equal the eager results."""
    from crfconv_amd import InferenceNet
    net = crf_net[0]
    fast = InferenceNet(net)
    static = batch._apply(lambda v: v.clone())
    second = make_batch(70)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fast(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = fast(static)
    var = net.conv1_1.lin_in.bn.batch_norm.running_var
    keep = var.clone()
    try:
        with torch.no_grad():
            static.load_(second)
            graph.replay()
            assert torch.equal(out, net(second))
            assert not torch.equal(out, net(batch))
            var.mul_(1.7).add_(0.05)
            graph.replay()
            changed = net(second)
            assert torch.equal(out, changed)
            var.copy_(keep)
            assert not torch.equal(changed, net(second))   # the change of the running statistics reached the logits
    finally:
        var.copy_(keep)


def test_scene_voter_takes_the_wrapper_as_its_net():
    """tests/test_gpu_scene_voter.py's small scene (two rooms, k = 4096, B = 2, 3 steps) through SceneVoter with InferenceNet(net13) and
    with net13 itself, the same seeds: equal vote tables, visits and logits; the wrapped model's mode is restored."""
    from crfconv_amd import InferenceNet, models
    from test_gpu_scene_voter import rooms, scene_voter_run
    torch.manual_seed(3)
    net13 = models.PointConvBig(6, 13, True, 3).to(DEV).eval()
    sd = S.fill_state_dict({k: tuple(v.shape) for k, v in net13.state_dict().items()}, 21)
    net13.load_state_dict(sd)
    sizes, k, Bv, steps = (9000, 2000), 4096, 2, 3
    sc = rooms(sizes, 51)
    sc[3][1] -= 4e-3
    plain = scene_voter_run(net13, sc, sizes, k, Bv, steps, 's3dis')
    fast = InferenceNet(net13)
    fast.train()                                           # left in training mode by the caller: SceneVoter switches and restores
    assert net13.training is True
    fused = scene_voter_run(fast, sc, sizes, k, Bv, steps, 's3dis')
    assert fast.training is True and net13.training is True
    fast.eval()
    assert net13.training is False
    for a, b in zip(plain[0] + plain[1], fused[0] + fused[1]):
        assert torch.equal(a, b)
    for (pa, ca, la), (pb, cb, lb) in zip(plain[2], fused[2]):
        assert torch.equal(pa, pb) and torch.equal(ca, cb) and torch.equal(la, lb)


@pytest.mark.parametrize('graphed', [False, True])
def test_vote_scene_takes_the_wrapper_as_its_net(graphed):
    from crfconv_amd import InferenceNet, models
    from crfconv_amd.sampling import VoteAccumulator, vote_scene
    from test_gpu_scene_voter import make_sampler, rooms
    torch.manual_seed(3)
    net = models.PointConvBig(6, 13, True, 3).to(DEV).eval()
    net.load_state_dict(S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 22))
    sizes, k = (6000, 6000), 4096
    sc = rooms(sizes, 52, box=(20.0, 20.0, 5.0))
    tables = []
    for model in (net, InferenceNet(net)):
        votes = VoteAccumulator(sizes, 13, device=DEV)
        vote_scene(make_sampler(sc, k, 'semantic3d'), model, votes, 3, generator=torch.Generator().manual_seed(9), graphed=graphed)
        votes.check()
        tables.append([p.clone() for p in votes.test_probs])
    for a, b in zip(*tables):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0


def test_refusals_and_the_hook_fallback(batch, crf_net):
    from crfconv_amd import InferenceNet, _lib
    net = crf_net[0]
    fast = InferenceNet(net)
    fast.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            fast(batch)
    finally:
        fast.eval()
    half = batch._apply(lambda v: v.clone())
    half.x = half.x.double()
    with pytest.raises(_lib.CrfConvError, match='float32'):
        fast(half)
    fired = []
    handle = net.conv1_1.lin_in.register_forward_hook(lambda mod, inp, out: fired.append(tuple(out.shape)))
    try:
        with torch.no_grad(), count_calls() as names:
            got = fast(batch)
            ref = net(batch)
    finally:
        handle.remove()
    assert len(fired) == 2 and torch.equal(got, ref)
    assert names['crfconv_linear_bn_act'] + names['crfconv_gemm_bn_act'] == 0      # the model's own forward ran, both times
    with torch.no_grad(), count_calls() as names:
        fast(batch)
    assert names['crfconv_linear_bn_act'] + names['crfconv_gemm_bn_act'] == 50


def test_a_layer_outside_the_fused_form_runs_its_own_module(batch):
    """A bias together with the BatchNorm, and a non-LeakyReLU activation: those layers run their module's eval forward, the rest stays fused."""
    from crfconv_amd import InferenceNet
    net, _ = make_net(True, 14)
    lin = net.conv1_2.lin_in.lin
    net.conv1_2.lin_in.lin = nn.Linear(lin.in_features, lin.out_features, bias=True).to(DEV)
    net.deconv1.out_nn.activation = nn.ReLU()
    net.eval()
    fast = InferenceNet(net)
    with torch.no_grad():
        ref = net(batch)
        with count_calls() as names:
            got = fast(batch)
    assert torch.equal(got, ref)
    assert names['crfconv_linear_bn_act'] + names['crfconv_gemm_bn_act'] == 48 and names['crfconv_bn_forward'] == 2
