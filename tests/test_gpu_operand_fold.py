"""The PointConv combine out = a2 U + (a2 shift + b2) V formed by the Linear kernel of lin_out while it loads its operand
(ops.CombineHandle; csrc/uv_fold.hpp) instead of by an elementwise launch of its own.  The folded forms do the same float operations on
the same values in the same order -- only a store -> load round trip disappears -- so fold on is compared against fold off on the same
inputs with torch.equal, except dW2 of the narrow PointConv (LDS float atomics: 1e-6, as in tests/test_gpu_mask_fold.py).
(The coarse fusion_nn without a materialised concatenation is not built: crfconv_cat2 / crfconv_split2 still run, and have no cases here.)"""

import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import DEV, assert_close, t

pytestmark = pytest.mark.gpu

FOLDED = {'fine': 'crfconv_linear_forward_uv', 'small': 'crfconv_mlp_small_forward_join_uv', 'tiled': 'crfconv_gemm_stats_uv'}
COUNTED = ('crfconv_pointconv_combine',) + tuple(FOLDED.values())


@pytest.fixture
def big_forms_from_4096(monkeypatch):
    """Rows from 4096 up take the row-streaming forms (shipped switch-over: 12 288 rows)."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'mfma_min_rows', 4096)


@pytest.fixture
def calls(monkeypatch):
    """Names of the counted launches issued through _lib.call, in order."""
    from crfconv_amd import _lib
    seen = []
    real = _lib.call

    def call(name, *a):
        if name in COUNTED:
            seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


# ------------------------------------------------------------------------------------------------------------------- one join

_CASES = {}


def _case(m, d, co):
    """A random cloud of m points with its K = 16 table, a PointConv layer of width d and lin_out d -> co with its BatchNorm and skip."""
    key = (m, d, co)
    if key not in _CASES:
        from crfconv_amd import ops
        g = torch.Generator().manual_seed(7 * m + 3 * d + co)
        pos = torch.rand(m, 3, generator=g).to(DEV)
        idx = torch.cdist(pos, pos).topk(16, dim=1, largest=False).indices
        table = ops.NeighborTable(idx.reshape(1, m, 16), m)
        mk = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
        prm = dict(W1=mk(d, 3), W2=mk(d, d) / d ** 0.5, W=mk(co, d) / d ** 0.5)
        prm = {k: torch.nn.Parameter(v) for k, v in prm.items()}
        bns = {}
        for name, c in (('bn1', d), ('bn2', d), ('bn', co)):
            bn = torch.nn.BatchNorm1d(c).to(DEV).train()
            with torch.no_grad():
                bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
                bn.bias.copy_(torch.randn(c, generator=g))
            bns[name] = bn
        _CASES[key] = dict(pos=pos, table=table, prm=prm, bns=bns, x=mk(m, d), skip=mk(m, co), go=mk(m, co))
    return _CASES[key]


def _nodes(out):
    """The autograd nodes behind `out`, by name."""
    found, stack, seen = {}, [out.grad_fn], set()
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        found.setdefault(f.name(), f)
        stack.extend(q for q, _ in f.next_functions)
    return found


def _run_join(case, fold, calls, via=None, off=None):
    """PointConv (training) -> the ResNet join on its output, one backward.  Returns every tensor the issue names.
    via: None = ops.mlp_block_join with the handle; 'alone' = ops.point_conv without a join behind it, then the join on the filled out.
    off: the set of consumer families switched off (ops.state.no_combine_fold), instead of all (fold False) or none (fold True)."""
    from crfconv_amd import ops
    prm, bns = case['prm'], case['bns']
    for p in prm.values():
        p.grad = None
    for bn in bns.values():
        bn.reset_running_stats()
        bn.weight.grad = bn.bias.grad = None
    x = case['x'].clone().requires_grad_(True)
    skip = case['skip'].clone().requires_grad_(True)
    old = ops.state.no_combine_fold
    ops.state.no_combine_fold = (not fold) if off is None else frozenset(off)
    del calls[:]
    try:
        args = (x, case['pos'], case['pos'], case['table'], prm['W1'], bns['bn1'], prm['W2'], bns['bn2'], True)
        if via == 'alone':
            y, handle = ops.point_conv(*args), None
            assert calls == ['crfconv_pointconv_combine']
            y_before = y.detach().clone()
        else:
            y, handle = ops.point_conv(*args, defer_combine=True)
            assert handle.pending == fold
        out = ops.mlp_block_join(y, prm['W'], bns['bn'], skip, 0.01, combine=handle)
        assert out is not None and (handle is None or not handle.pending)
        if via == 'alone':
            assert torch.equal(y_before, y.detach())
        seen = list(calls)
        nodes = _nodes(out)                                   # (saved tensors are released by the backward)
        join = nodes.get('_MLPBlockJoinBackward') or nodes['_MLPSmallJoinBackward']
        jx, _, jy, jcoef, jout = join.saved_tensors
        _, _, _, _, _, _, _, a2, b2, _, _, aux2, _, _, _ = nodes['_PointConvBackward'].saved_tensors
        out.backward(case['go'])
    finally:
        ops.state.no_combine_fold = old
    res = {'out': out.detach(), 'Y': jy, 'coef': jcoef, 'pc_out': y.detach(), 'join_x': jx, 'a2': a2, 'b2': b2, 'aux2': aux2,
           'dx': x.grad, 'dskip': skip.grad}
    for k, p in prm.items():
        res['d' + k] = p.grad
    for k, bn in bns.items():
        res.update({k + '.rm': bn.running_mean, k + '.rv': bn.running_var, k + '.dgamma': bn.weight.grad, k + '.dbeta': bn.bias.grad})
    return {k: v.detach().clone() for k, v in res.items()}, seen, type(join).__name__


def _assert_equal(got, ref, d):
    assert got.keys() == ref.keys()
    for k in got:
        assert torch.isfinite(got[k]).all(), k
        if k == 'dW2' and d <= 16:
            assert_close(got[k], ref[k], 1e-6, k)            # narrow PointConv: LDS float atomics in its parameter pass
        else:
            assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))


def _check_family(m, d, co, family, node, calls):
    case = _case(m, d, co)
    ref, seen_off, node_off = _run_join(case, False, calls)
    got, seen_on, node_on = _run_join(case, True, calls)
    assert node_on == node_off == node
    assert seen_off.count('crfconv_pointconv_combine') == 1 and not any(n in seen_off for n in FOLDED.values())
    assert seen_on == [FOLDED[family]], seen_on
    assert torch.equal(got['pc_out'], got['join_x'])          # the join's operand IS the side-written out
    _assert_equal(got, ref, d)


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('d,co', [(8, 32), (16, 64)])
def test_fine_join_forms_the_combine_on_operand_load(d, co, calls):
    """Row-streaming Linear, 4100 rows: a partial 16-row group, several workgroups."""
    _check_family(4100, d, co, 'fine', '_MLPBlockJoinBackward', calls)


@pytest.mark.parametrize('m', [37, 200])
@pytest.mark.parametrize('d,co', [(64, 256), (128, 512)])
def test_one_launch_coarse_join_forms_the_combine_on_operand_load(m, d, co, calls):
    """One-launch Linear + BatchNorm + join: a partial 64-row tile, several column tiles -- out is stored by column tile 0 alone."""
    from crfconv_amd import _lib, ops
    assert not ops.state.small_mlp_disabled and _lib.load().crfconv_mlp_small_supported(m, d, co) == 1
    _check_family(m, d, co, 'small', '_MLPSmallJoinBackward', calls)
    assert int(ops.gridsync_ws(DEV).abs().sum()) == 0


def test_tiled_coarse_join_forms_the_combine_on_operand_load(calls):
    """4100 rows with the shipped switch-over: past the one-launch kernel's row limit, below the row-streaming forms."""
    from crfconv_amd import _lib, ops
    assert ops.state.mfma_min_rows == 12288 and _lib.load().crfconv_mlp_small_supported(4100, 32, 128) == 0
    _check_family(4100, 32, 128, 'tiled', '_MLPSmallJoinBackward', calls)


@pytest.mark.parametrize('family', ['fine', 'small', 'tiled'])
def test_family_switch_leaves_the_other_families_folded(family, calls, monkeypatch):
    """ops.state.no_combine_fold as a set of families: that family launches the combine, the result is the folded one."""
    from crfconv_amd import ops
    m, d, co = {'fine': (4100, 8, 32), 'small': (200, 64, 256), 'tiled': (4100, 32, 128)}[family]
    if family == 'fine':
        monkeypatch.setattr(ops.state, 'mfma_min_rows', 4096)
    case = _case(m, d, co)
    ref, _, _ = _run_join(case, True, calls)
    got, seen, _ = _run_join(case, True, calls, off={family})
    assert seen == ['crfconv_pointconv_combine'], seen
    _assert_equal(got, ref, d)
    got, seen, _ = _run_join(case, True, calls, off={'fine', 'small', 'tiled'} - {family})
    assert seen == [FOLDED[family]], seen
    _assert_equal(got, ref, d)


# ------------------------------------------------------------------------------------------------------------------- fallbacks

@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('m,d,co', [(4100, 8, 32), (200, 64, 256)])
def test_point_conv_on_its_own_fills_out_with_the_old_combine(m, d, co, calls):
    """ops.point_conv without a join behind it: out is filled when it returns and equals the folded result."""
    case = _case(m, d, co)
    ref, _, _ = _run_join(case, True, calls)
    got, seen, _ = _run_join(case, True, calls, via='alone')
    assert seen == ['crfconv_pointconv_combine'], seen
    _assert_equal(got, ref, d)


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('m,d,co', [(4100, 16, 64), (37, 128, 512)])
def test_no_join_falls_back_to_the_old_combine(m, d, co, calls, monkeypatch):
    """state.no_join: the block's tail runs as separate nodes; the handle launches the combine before lin_out reads out."""
    from crfconv_amd import ops
    from crfconv_amd.models.common import MLP, mlp_join
    case = _case(m, d, co)
    ref, _, _ = _run_join(case, True, calls)
    prm, bns = case['prm'], case['bns']
    lin_out = MLP(d, co, activation=None).to(DEV).train()
    with torch.no_grad():
        lin_out.lin.weight.copy_(prm['W'])
        lin_out.bn.batch_norm.weight.copy_(bns['bn'].weight)
        lin_out.bn.batch_norm.bias.copy_(bns['bn'].bias)
    for bn in bns.values():
        bn.reset_running_stats()
    monkeypatch.setattr(ops.state, 'no_join', True)
    del calls[:]
    y, handle = ops.point_conv(case['x'], case['pos'], case['pos'], case['table'], prm['W1'], bns['bn1'], prm['W2'], bns['bn2'], True,
                               defer_combine=True)
    assert handle.pending
    out = mlp_join(lin_out, y, case['skip'], 0.01, combine=handle)
    assert not handle.pending and calls == ['crfconv_pointconv_combine'], calls
    assert torch.equal(y.detach(), ref['pc_out'])
    assert torch.equal(bns['bn2'].running_mean, ref['bn2.rm']) and torch.equal(bns['bn2'].running_var, ref['bn2.rv'])
    assert_close(out, ref['out'], 1e-5, 'out')               # another node sequence behind the same operand


# ---------------------------------------------------------------------------------------------------------------- whole network

@pytest.mark.usefixtures('big_forms_from_4096')
def test_whole_network_launch_counts(calls, monkeypatch):
    """One training forward + backward of PointConvBig(6, 13, use_crf=True, steps=2) on two 4096-point clouds: no combine launch with
    the folds on, ten with them off; equal logits and gradients."""
    import crfconv_amd
    from crfconv_amd import models, ops, train
    B, N = 2, 4096
    pos = np.stack([S.make_cloud(20 + b, N, box=(2.0, 2.0, 1.0)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(20, 'rgb', (B, N, 3), 0, 1)], -1).astype(np.float32)
    labels = S.integers(20, 'y', (B, N), 0, 14)
    choices, n = [], N
    for i, r in enumerate((4, 4, 4, 4, 2)):
        choices.append(torch.from_numpy(S.permutation(20, 'c%d' % i, n)[: n // r]))
        n //= r
    data = crfconv_amd.multiscale_compute(t(pos), x=t(feats), choices=choices)
    net = models.PointConvBig(6, 13, use_crf=True, steps=2)
    sd = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 5)
    net = net.to(DEV).train()
    y = torch.from_numpy(labels.reshape(-1)).long().to(DEV) - 1
    res, counts = {}, {}
    for fold in (True, False):
        monkeypatch.setattr(ops.state, 'no_combine_fold', not fold)
        net.load_state_dict(sd)
        for p in net.parameters():
            p.grad = None
        del calls[:]
        with train.no_autograph():
            logits = net(data)
            loss = torch.nn.functional.cross_entropy(logits, y, ignore_index=-1)
            loss.backward()
        counts[fold] = {n: calls.count(n) for n in COUNTED}
        res[fold] = (logits.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
                     {k: v.detach().clone() for k, v in net.state_dict().items()})
    assert counts[False]['crfconv_pointconv_combine'] == 10 and sum(counts[False][n] for n in FOLDED.values()) == 0, counts
    assert counts[True]['crfconv_pointconv_combine'] == 0 and sum(counts[True][n] for n in FOLDED.values()) == 10, counts
    assert counts[True][FOLDED['fine']] == 2 and counts[True][FOLDED['small']] == 8, counts      # level 0 streams its 8192 rows
    assert torch.equal(res[True][0], res[False][0])
    for k, a in res[True][2].items():
        assert torch.equal(a, res[False][2][k]), k                             # running statistics, step counters
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) > 100
    for k, a in res[True][1].items():
        b = res[False][1][k]
        if 'point_conv' in k and 'weight_nn.1.lin' in k:
            assert_close(a, b, 1e-6, k)
        else:
            assert torch.equal(a, b), (k, float((a - b).abs().max()))
