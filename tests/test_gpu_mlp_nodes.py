"""Every fused Linear -> BatchNorm(train) -> (LeakyReLU | + skip | dropout | max-pool) node of ops.mlp through its public wrapper, forward
plus backward in the three ways a parameter gradient leaves a node: returned to autograd, inside ``deferred_weight_grads()`` (finished
by the launches at the end of the pass), inside ``deferred_weight_grads(sink=bucket.view_of)`` (written into a flat bucket).  The
delivery mode changes no launch that produces an output, an input gradient or a running statistic, so those are compared with
torch.equal; the parameter gradients agree to 1e-6 (the deferred weight gradients are summed in another launch)."""

import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

MODES = ('autograd', 'deferred', 'bucket')
M_BIG, M_SMALL = 4100, 37          # a partial 16-row group and several workgroups / far below every coarse-level limit


@pytest.fixture
def big_forms_from_4096(monkeypatch):
    """4100 rows take the row-streaming forms (shipped switch-over: 12 288 rows), 37 rows the coarse ones."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'mfma_min_rows', 4096)


class _Block(torch.nn.Module):
    """The parameters of one family: a Linear weight per (Ci, Co) of `widths`, a BatchNorm behind the first `n_bn` of them (default: all),
    a bias `b` for the last Linear if asked for."""

    def __init__(self, gen, widths, n_bn=None, bias=False):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(co, ci, generator=gen) / ci ** 0.5) for ci, co in widths])
        self.b = torch.nn.Parameter(torch.randn(widths[-1][1], generator=gen)) if bias else None
        self.bn = torch.nn.ModuleList([torch.nn.BatchNorm1d(co) for _, co in widths[:n_bn]])
        with torch.no_grad():
            for bn in self.bn:
                bn.weight.copy_(torch.rand(bn.num_features, generator=gen) + 0.5)
                bn.bias.copy_(torch.randn(bn.num_features, generator=gen) * 0.3)


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen).to(DEV)


def _f_block(gen, ci=24, co=64, m=M_BIG):
    from crfconv_amd import ops
    blk = _Block(gen, [(ci, co)])
    xs = [_rand(gen, m, ci)]
    assert ops.mlp_block_ok(xs[0], blk.w[0], None, blk.bn[0], True)
    return blk, xs, lambda x: [ops.mlp_block(x, blk.w[0], blk.bn[0], 0.1)]


def _f_join(gen, ci=64, co=16, m=M_BIG):
    from crfconv_amd import ops
    blk = _Block(gen, [(ci, co)])
    xs = [_rand(gen, m, ci), _rand(gen, m, co)]
    return blk, xs, lambda x, skip: [ops.mlp_block_join(x, blk.w[0], blk.bn[0], skip, 0.01)]


def _f_masked_fork(gen):
    """A join (24 -> 64) whose output goes into a forking block (64 -> 16) that was told it writes the join's total gradient: the
    block's dX carries the join's LeakyReLU mask, the alias has a second consumer."""
    from crfconv_amd import ops
    blk = _Block(gen, [(24, 64), (64, 16)])
    xs = [_rand(gen, M_BIG, 24), _rand(gen, M_BIG, 64)]

    def fwd(x, skip):
        hs = ops.JoinMask()
        h = ops.mlp_block_join(x, blk.w[0], blk.bn[0], skip, 0.01, mask=hs)
        out, alias = ops.mlp_block(h, blk.w[1], blk.bn[1], 0.1, fork=True, input_mask=hs)
        assert hs.folded and hs.slope == pytest.approx(0.01)
        return [out, alias * 0.5]
    return blk, xs, fwd


_TABLE = {}


def _pool_table(gen):
    """1025 targets with K = 8 neighbours among 4100 sources, built once."""
    if not _TABLE:
        from crfconv_amd import ops
        idx = torch.randint(0, M_BIG, (1, M_BIG // 4, 8), generator=gen)
        _TABLE['t'] = ops.NeighborTable(idx.to(DEV), M_BIG)
    return _TABLE['t']


def _f_pool(gen):
    from crfconv_amd import ops
    table = _pool_table(torch.Generator().manual_seed(77))
    blk = _Block(gen, [(24, 64)])
    xs = [_rand(gen, M_BIG, 24)]

    def fwd(x):
        out, alias = ops.mlp_block_pool(x, blk.w[0], blk.bn[0], table, fork=True)
        return [out, alias * 0.5]
    return blk, xs, fwd


def _f_dropout(gen):
    from crfconv_amd import ops
    blk = _Block(gen, [(24, 64)])
    return blk, [_rand(gen, M_BIG, 24)], lambda x: [ops.mlp_block_dropout(x, blk.w[0], blk.bn[0], 0.1, 0.5)]


def _f_dropout_linear(gen):
    from crfconv_amd import ops
    blk = _Block(gen, [(24, 64), (64, 16)], n_bn=1, bias=True)
    return blk, [_rand(gen, M_BIG, 24)], lambda x: [ops.mlp_dropout_linear(x, blk.w[0], blk.bn[0], 0.1, 0.5, blk.w[1], blk.b, recompute=False)]


def _f_head_recompute(gen):
    """(12288, 16, 8) of test_classifier_head_recompute: the smallest of its row counts, taken by crfconv_head_supported."""
    from crfconv_amd import _lib, ops
    m, ci, co, c2 = 12288, 16, 128, 8
    assert _lib.load().crfconv_head_supported(m, ci, co, c2)
    blk = _Block(gen, [(ci, co), (co, c2)], n_bn=1)
    return blk, [_rand(gen, m, ci)], lambda x: [ops.mlp_dropout_linear(x, blk.w[0], blk.bn[0], 0.1, 0.5, blk.w[1], None, recompute=True)]


def _f_cat(gen):
    from crfconv_amd import ops
    blk = _Block(gen, [(24, 64)])
    xs = [_rand(gen, M_BIG, 12), _rand(gen, M_BIG, 12)]
    return blk, xs, lambda xa, xb: [ops.mlp_block_cat(xa, xb, blk.w[0], blk.bn[0], True, 0.1)]


def _f_group(gen):
    """Two blocks on the SAME 37 x 64 tensor, the first forking."""
    from crfconv_amd import ops
    blk = _Block(gen, [(64, 16), (64, 64)])
    xs = [_rand(gen, M_SMALL, 64)]

    def fwd(x):
        res = ops.mlp_group([(x, blk.w[0], blk.bn[0], 0.1, True), (x, blk.w[1], blk.bn[1], 1.0, False)], shared=True)
        assert res is not None
        (o0, alias), o1 = res
        return [o0, alias * 0.5, o1]
    return blk, xs, fwd


# family -> (builder, the node its graph must hold)
FAMILIES = {
    'block_24_64': (_f_block, '_MLPBlockBackward'),
    'block_64_16': (lambda g: _f_block(g, 64, 16), '_MLPBlockBackward'),
    'block_fork_masked': (_f_masked_fork, '_MLPBlockBackward'),
    'join_64_16': (_f_join, '_MLPBlockJoinBackward'),
    'join_24_64': (lambda g: _f_join(g, 24, 64), '_MLPBlockJoinBackward'),
    'pool_fork': (_f_pool, '_MLPBlockPoolBackward'),
    'dropout': (_f_dropout, '_MLPBlockDropoutBackward'),
    'dropout_linear': (_f_dropout_linear, '_MLPDropoutLinearBackward'),
    'head_recompute': (_f_head_recompute, '_HeadRecomputeBackward'),
    'cat': (_f_cat, '_MLPBlockCatBackward'),
    'coarse_block': (lambda g: _f_block(g, 24, 64, M_SMALL), '_MLPSmallBackward'),
    'coarse_join': (lambda g: _f_join(g, 64, 16, M_SMALL), '_MLPSmallJoinBackward'),
    'coarse_group': (_f_group, '_MLPSmallGroupBackward'),
}


def build_family(name):
    """(block, inputs, forward, the block's state at the start) of one family, from its own seed."""
    gen = torch.Generator().manual_seed(1000 + sorted(FAMILIES).index(name))
    blk, xs, fwd = FAMILIES[name][0](gen)
    blk = blk.to(DEV).train()
    return blk, xs, fwd, {k: v.clone() for k, v in blk.state_dict().items()}


def _node_names(outs):
    seen, stack = set(), [o.grad_fn for o in outs]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        stack.extend(q for q, _ in f.next_functions)
    return {f.name() for f in seen}


def run_family(case, mode):
    """One forward + backward from the case's inputs and parameter values.  The dropout seed is a function of torch.initial_seed() and
    the mask of the BatchNorm's step counter: both are put back first, so the three runs draw the same mask."""
    from crfconv_amd import distributed, ops
    blk, xs0, fwd, state0 = case
    torch.manual_seed(7)
    blk.load_state_dict(state0)                            # running statistics and num_batches_tracked as at the start
    for p in blk.parameters():
        p.grad = None
    xs = [v.clone().requires_grad_(True) for v in xs0]
    outs = fwd(*xs)
    assert all(o is not None for o in outs)
    gen = torch.Generator().manual_seed(99)
    gouts = [_rand(gen, *o.shape) for o in outs]
    res = {'nodes': _node_names(outs), 'bucket': None}
    if mode == 'autograd':
        torch.autograd.backward(outs, gouts)
    elif mode == 'deferred':
        with ops.deferred_weight_grads():
            torch.autograd.backward(outs, gouts)
    else:
        bucket = res['bucket'] = distributed.FlatGradAllReduce(blk)
        with ops.deferred_weight_grads(sink=bucket.view_of):
            torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    res['same'] = {'out%d' % i: o.detach().clone() for i, o in enumerate(outs)}
    res['same'].update({'dx%d' % i: v.grad.clone() for i, v in enumerate(xs)})
    res['same'].update({k: v.clone() for k, v in blk.state_dict().items() if 'running' in k or 'num_batches' in k})
    res['pgrad'] = {k: p.grad.clone() for k, p in blk.named_parameters()}
    res['grad_ptr'] = {k: p.grad.data_ptr() for k, p in blk.named_parameters()}
    return res


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('name', list(FAMILIES))
def test_node_results_do_not_depend_on_how_parameter_gradients_are_delivered(name):
    case = build_family(name)
    blk = case[0]
    ref = run_family(case, 'autograd')
    assert FAMILIES[name][1] in ref['nodes'], ref['nodes']
    assert all(torch.isfinite(v).all() for v in ref['same'].values()) and all(torch.isfinite(v).all() for v in ref['pgrad'].values())
    for mode in MODES[1:]:
        got = run_family(case, mode)
        assert FAMILIES[name][1] in got['nodes'], got['nodes']
        assert got['same'].keys() == ref['same'].keys()
        for k, v in ref['same'].items():
            assert torch.equal(got['same'][k], v), (mode, k, float((got['same'][k].double() - v.double()).abs().max()))
        assert got['pgrad'].keys() == ref['pgrad'].keys() and len(ref['pgrad']) >= 3
        for k, v in ref['pgrad'].items():
            err, bound = float((got['pgrad'][k] - v).abs().max()), 1e-6 * float(v.abs().max()) + 1e-9
            print('%s %s %s: |d| %.3e bound %.3e' % (name, mode, k, err, bound))
            assert err <= bound, (mode, k, err, bound)
        if mode == 'bucket':
            for k, p in blk.named_parameters():
                assert got['grad_ptr'][k] == got['bucket'].view_of(p).data_ptr(), k
