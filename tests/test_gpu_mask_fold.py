"""The LeakyReLU mask of a ResNet join's backward, g1 = g lrelu'(out), applied by the kernel that WRITES g (the dX product of the next
block's lin_in, or the sum launch of its shared group) instead of by a pass of its own (ops.JoinMask).  The folded path does the same
float operations on the same values -- only a store -> load round trip disappears -- so everything is compared with torch.equal, except
dW2 of the narrow PointConv (LDS float atomics: 1e-6, as in tests/test_gpu_model.py)."""

import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import DEV, assert_close, t

pytestmark = pytest.mark.gpu


@pytest.fixture
def big_forms_from_4096(monkeypatch):
    """B N = 8192 rows at level 0 take the row-streaming forms (shipped switch-over: 12 288 rows), the 2048 of level 1 the small ones."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'mfma_min_rows', 4096)


@pytest.fixture
def mask_passes(monkeypatch):
    """Counts the crfconv_add_lrelu_backward launches issued through _lib.call."""
    from crfconv_amd import _lib
    seen = []
    real = _lib.call

    def call(name, *a):
        if name == 'crfconv_add_lrelu_backward':
            seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


def _signed_zero_ref(M, C, g):
    """A mask reference with negative values, +0.0 and -0.0 (first rows and the last, partial, 16-row group)."""
    ref = torch.randn(M, C, generator=g)
    ref[0, 0], ref[0, 1], ref[1, C - 1] = 0.0, -0.0, -0.0
    ref[M - 1, C - 1], ref[M - 1, 0], ref[M - 2, 2] = 0.0, -0.0, 0.0
    assert (ref < 0).any() and bool(torch.signbit(ref[0, 1])) and not bool(torch.signbit(ref[0, 0]))
    return ref.to(DEV)


# ------------------------------------------------------------------------------------------------------------------ kernel level

@pytest.mark.parametrize('with_add', [True, False])
@pytest.mark.parametrize('mslope', [0.01, 0.1])
@pytest.mark.parametrize('ci,co', [(32, 8), (64, 16), (128, 32), (24, 8), (16, 64)])      # (16, 64): one 16-column output tile per workgroup
def test_fine_dx_masked_epilogue_equals_product_then_mask_pass(ci, co, mslope, with_add):
    """crfconv_mlp_backward_add_mask against crfconv_mlp_backward_add followed by crfconv_add_lrelu_backward(dX, x): 4100 rows (a partial
    16-row group, several workgroups), the widths of the fine-level lin_in blocks, with the alias gradient and without."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.ops import ptr, stream_ptr
    lib = _lib.load()
    M = 4100
    g = torch.Generator().manual_seed(ci * 131 + co)
    x = _signed_zero_ref(M, ci, g)
    W = (torch.randn(co, ci, generator=g) / ci ** 0.5).to(DEV)
    gA = torch.randn(M, co, generator=g).to(DEV)
    add = torch.randn(M, ci, generator=g).to(DEV) if with_add else None
    gamma, beta = (torch.rand(co, generator=g) + 0.5).to(DEV), torch.randn(co, generator=g).to(DEV)
    rm, rv = torch.zeros(co, device=DEV), torch.ones(co, device=DEV)
    y, rec = ops._mfma_matmul(x, W, None, False, True)
    coef = torch.empty(4 * co, device=DEV)
    out = torch.empty_like(y)
    _lib.call('crfconv_bn_apply_from_records', ptr(rec), rec.shape[0], ptr(y), M, co, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5,
              None, 0.1, ptr(coef), ptr(out), stream_ptr())
    assert lib.crfconv_mlp_backward_supported(M, ci, co) == 1
    nbytes = lib.crfconv_mlp_backward_workspace(M, ci, co)

    def run(masked):
        dX = torch.full((M, ci), float('nan'), device=DEV)
        dW, dg, db = torch.empty(co, ci, device=DEV), torch.empty(co, device=DEV), torch.empty(co, device=DEV)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        if masked:
            _lib.call('crfconv_mlp_backward_add_mask', ptr(gA), ptr(y), ptr(x), ptr(W), ptr(coef), 0.1, M, ci, co, ptr(add), mslope, ptr(dX),
                      ptr(dW), ptr(dg), ptr(db), ptr(ws), nbytes, ops._mlp_ticket(DEV), stream_ptr())
            return dX, dW, dg, db
        _lib.call('crfconv_mlp_backward_add', ptr(gA), ptr(y), ptr(x), ptr(W), ptr(coef), 0.1, M, ci, co, ptr(add), ptr(dX),
                  ptr(dW), ptr(dg), ptr(db), ptr(ws), nbytes, ops._mlp_ticket(DEV), stream_ptr())
        g1 = torch.empty_like(dX)
        _lib.call('crfconv_add_lrelu_backward', ptr(dX), ptr(x), dX.numel(), mslope, ptr(g1), stream_ptr())
        return g1, dW, dg, db, dX
    ref, got = run(False), run(True)
    assert torch.isfinite(got[0]).all()
    for name, a, b in zip(('dX', 'dW', 'dgamma', 'dbeta'), got, ref):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert torch.equal(got[0], torch.where(x > 0, ref[4], mslope * ref[4])) and not torch.equal(got[0], ref[4])      # -0.0 and +0.0: slope side


@pytest.mark.parametrize('ci,co', [(6, 32), (22, 8)])
def test_fine_dx_add_epilogue_on_unaligned_inputs_equals_product_then_add(ci, co):
    """crfconv_mlp_backward_add on a block whose input width is no multiple of 4 -- the element-wise dX product, which the masked form
    above refuses -- against crfconv_mlp_backward followed by dX + add: 133 rows (several workgroups, a partial last 16-row group), one
    and two 16-column output tiles per workgroup."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.ops import ptr, stream_ptr
    lib = _lib.load()
    M = 133
    g = torch.Generator().manual_seed(ci * 131 + co)
    x = torch.randn(M, ci, generator=g).to(DEV)
    W = (torch.randn(co, ci, generator=g) / ci ** 0.5).to(DEV)
    gA = torch.randn(M, co, generator=g).to(DEV)
    add = torch.randn(M, ci, generator=g).to(DEV)
    gamma, beta = (torch.rand(co, generator=g) + 0.5).to(DEV), torch.randn(co, generator=g).to(DEV)
    rm, rv = torch.zeros(co, device=DEV), torch.ones(co, device=DEV)
    y, rec = ops._mfma_matmul(x, W, None, False, True)
    coef = torch.empty(4 * co, device=DEV)
    out = torch.empty_like(y)
    _lib.call('crfconv_bn_apply_from_records', ptr(rec), rec.shape[0], ptr(y), M, co, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5,
              None, 0.1, ptr(coef), ptr(out), stream_ptr())
    assert lib.crfconv_mlp_backward_supported(M, ci, co) == 1
    nbytes = lib.crfconv_mlp_backward_workspace(M, ci, co)

    def run(name, *addend):
        dX = torch.full((M, ci), float('nan'), device=DEV)
        dW, dg, db = torch.empty(co, ci, device=DEV), torch.empty(co, device=DEV), torch.empty(co, device=DEV)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call(name, ptr(gA), ptr(y), ptr(x), ptr(W), ptr(coef), 0.1, M, ci, co, *addend, ptr(dX), ptr(dW), ptr(dg), ptr(db), ptr(ws),
                  nbytes, ops._mlp_ticket(DEV), stream_ptr())
        return dX, dW, dg, db
    ref, got = run('crfconv_mlp_backward'), run('crfconv_mlp_backward_add', ptr(add))
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], ref[0] + add), float((got[0] - (ref[0] + add)).abs().max())
    for name, a, b in zip(('dW', 'dgamma', 'dbeta'), got[1:], ref[1:]):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


@pytest.mark.parametrize('one_launch', [True, False])
@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('with_add', [True, False])
@pytest.mark.parametrize('M', [100, 2560])
def test_coarse_dx_product_masks_per_job(M, with_add, masked, one_launch, monkeypatch):
    """Two jobs of widths (64, 16) and (256, 64) in ONE crfconv_mlp_small_backward_jobs(_one_launch) call, job `masked` with a mask
    reference and the other without: equal to the unmasked call followed by crfconv_add_lrelu_backward on that job's dX alone."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.ops import ptr, stream_ptr
    lib = _lib.load()
    monkeypatch.setattr(ops.state, 'small_bwd_one_launch', one_launch)
    assert not ops.state.small_mlp_disabled
    g = torch.Generator().manual_seed(M + masked)
    shapes = [(64, 16), (256, 64)]
    mslope = 0.01
    probs = []
    for ci, co in shapes:
        yv = (torch.randn(M, co, generator=g) * 1.5 + 0.3).to(DEV)
        gA = torch.randn(M, co, generator=g).to(DEV)
        W = (torch.randn(co, ci, generator=g) / co ** 0.5).to(DEV)
        add = torch.randn(M, ci, generator=g).to(DEV) if with_add else None
        mean, var = yv.double().mean(0), yv.double().var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        coef = torch.cat([rstd, -rstd * mean, mean, rstd]).float().contiguous()
        probs.append((yv, gA, W, add, coef, _signed_zero_ref(M, ci, g)))

    def run(fold):
        outs, jobs = [], (_lib.MlpBwdJob * 2)()
        for i, ((ci, co), (yv, gA, W, add, coef, ref)) in enumerate(zip(shapes, probs)):
            nb = lib.crfconv_mlp_small_backward_workspace(M, co)
            o = (torch.full((M, co), float('nan'), device=DEV), torch.full((M, ci), float('nan'), device=DEV), torch.empty(co, device=DEV),
                 torch.empty(co, device=DEV), torch.empty(nb, dtype=torch.uint8, device=DEV))
            outs.append(o)
            mref = ref.data_ptr() if (fold and i == masked) else None
            jobs[i] = _lib.MlpBwdJob(gA.data_ptr(), yv.data_ptr(), coef.data_ptr(), W.data_ptr(), None if add is None else add.data_ptr(),
                                     M, ci, co, 1, 0.1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), nb,
                                     mref, mslope)
        ops._small_bwd_jobs(jobs, 2, DEV, stream_ptr())
        res = [list(o[:4]) for o in outs]
        if not fold:
            g1 = torch.empty_like(res[masked][1])
            _lib.call('crfconv_add_lrelu_backward', ptr(res[masked][1]), ptr(probs[masked][5]), g1.numel(), mslope, ptr(g1), stream_ptr())
            res[masked][1] = g1
        return res
    ref, got = run(False), run(True)
    for j in range(2):
        assert torch.isfinite(got[j][1]).all()
        for name, a, b in zip(('gY', 'dX', 'dgamma', 'dbeta'), got[j], ref[j]):
            assert torch.equal(a, b), (j, name, float((a - b).abs().max()))
    assert int(ops.gridsync_ws(DEV).abs().sum()) == 0


def test_masked_sum_equals_sum_then_mask_pass():
    """crfconv_add_mask(a, b, ref) against crfconv_add_lrelu(a, b, slope 1) followed by crfconv_add_lrelu_backward, 100 x 64."""
    from crfconv_amd import _lib
    from crfconv_amd.ops import ptr, stream_ptr
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(100, 64, generator=g).to(DEV), torch.randn(100, 64, generator=g).to(DEV)
    ref = _signed_zero_ref(100, 64, g)
    tot, want, got = torch.empty_like(a), torch.empty_like(a), torch.full_like(a, float('nan'))
    _lib.call('crfconv_add_lrelu', ptr(a), ptr(b), a.numel(), 1.0, ptr(tot), stream_ptr())
    _lib.call('crfconv_add_lrelu_backward', ptr(tot), ptr(ref), a.numel(), 0.01, ptr(want), stream_ptr())
    _lib.call('crfconv_add_mask', ptr(a), ptr(b), ptr(ref), a.numel(), 0.01, ptr(got), stream_ptr())
    assert torch.equal(got, want)
    assert torch.equal(got, torch.where(ref > 0, a + b, 0.01 * (a + b)))


# ------------------------------------------------------------------------------------------------------------------- block level

_SCENE = {}


def _scene():
    """The multiscale geometry of two 4096-point clouds, computed once for the tests of this module."""
    if not _SCENE:
        import crfconv_amd
        B, N = 2, 4096
        pos = np.stack([S.make_cloud(330 + b, N, box=(2, 2, 1)) for b in range(B)])
        _SCENE['data'] = crfconv_amd.multiscale_compute(t(pos), generator=torch.Generator().manual_seed(4))
    return _SCENE['data']


# (level, width in, width out of the second block, second block strided): the first block is an identity block of width `cin`
CHAINS = {'fine_identity': (0, 32, 32, False), 'fine_strided': (0, 32, 64, True),
          'coarse_identity': (1, 64, 64, False), 'coarse_grouped': (1, 64, 128, True)}


def _chain(name):
    from crfconv_amd.models.point_conv_big import ResNetBBlock
    lv, cin, cout, strided = CHAINS[name]
    data = _scene()
    lvl, nxt = data.multiscale[lv], data.multiscale[lv + 1]
    torch.manual_seed(cin + cout + lv)
    blocks = (ResNetBBlock(cin, cin).to(DEV).train(), ResNetBBlock(cin, cout).to(DEV).train())
    geo_a = (lvl.pos, lvl.neighbor_idx)
    geo_b = ((lvl.pos, nxt.pos), lvl.sub_idx) if strided else geo_a
    n_in, n_out = lvl.pos.shape[1], (nxt.pos.shape[1] if strided else lvl.pos.shape[1])
    g = torch.Generator().manual_seed(29)
    x0 = torch.randn(2, n_in, cin, generator=g).to(DEV)
    go = torch.randn(2, n_out, cout, generator=g).to(DEV)
    ga = torch.randn(2, n_in, cin, generator=g).to(DEV)        # gradient of the alias' second consumer (the decoder's place)
    return blocks, geo_a, geo_b, strided, x0, go, ga


def _run_chain(chain, x, wired=True, outside_consumer=False):
    """Two consecutive blocks as PointConvResNet._forward wires them; strided: the second returns the input alias, which gets a second
    consumer.  Returns (out, input gradient of x, parameter gradients, the handshake)."""
    from crfconv_amd import ops
    (blk_a, blk_b), geo_a, geo_b, strided, _, go, ga = chain
    for blk in (blk_a, blk_b):
        for p in blk.parameters():
            p.grad = None
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.reset_running_stats()
    x.grad = None
    hs = ops.JoinMask()
    h = blk_a(x * 1.0, geo_a[0], geo_a[1], join_mask=hs)
    outs, grads = [], []
    if outside_consumer:
        outs.append(h * 2.0)
        grads.append(ga)
    mask = hs if wired else None
    if strided:
        out, alias = blk_b(h, geo_b[0], geo_b[1], return_input_alias=True, input_mask=mask)
        outs += [out, alias * 0.5]
        grads += [go, ga]
    else:
        out = blk_b(h, geo_b[0], geo_b[1], input_mask=mask)
        outs.append(out)
        grads.append(go)
    torch.autograd.backward(outs, grads)
    gp = {'%d.%s' % (i, k): p.grad.clone() for i, blk in enumerate((blk_a, blk_b)) for k, p in blk.named_parameters()}
    return out.detach().clone(), x.grad.clone(), gp, hs


def _assert_same(a, b):
    (o1, gx1, gp1, _), (o2, gx2, gp2, _) = a, b
    assert torch.equal(o1, o2)
    assert torch.equal(gx1, gx2), float((gx1 - gx2).abs().max())
    for k in gp1:
        if 'point_conv' in k and 'weight_nn.1.lin' in k:
            assert_close(gp1[k], gp2[k], 1e-6, k)                # dW2 of a narrow PointConv: LDS float atomics
        else:
            assert torch.equal(gp1[k], gp2[k]), k


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('name', list(CHAINS))
def test_two_block_chain_fold_on_equals_fold_off(name, mask_passes, monkeypatch):
    """Fold on against fold off: out, the input gradient and the parameter gradients are equal, and one mask pass fewer runs (the
    second block's join keeps its own: nobody was told to write its gradient masked)."""
    from crfconv_amd import ops
    chain = _chain(name)
    x = chain[4].clone().requires_grad_(True)
    lv, cin, cout, strided = CHAINS[name]
    res, counts = {}, {}
    for fold in (True, False):
        monkeypatch.setattr(ops.state, 'no_mask_fold', not fold)
        del mask_passes[:]
        res[fold] = _run_chain(chain, x)
        counts[fold] = len(mask_passes)
        assert res[fold][3].folded == fold
    assert counts == {True: 1, False: 2}, counts
    _assert_same(res[True], res[False])
    # the forms the issue names were the ones that ran
    names = set()
    monkeypatch.setattr(ops.state, 'no_mask_fold', False)
    hs = ops.JoinMask()
    (blk_a, blk_b), geo_a, geo_b = chain[0], chain[1], chain[2]
    h = blk_a(x * 1.0, geo_a[0], geo_a[1], join_mask=hs)
    out = blk_b(h, geo_b[0], geo_b[1], return_input_alias=strided, input_mask=hs)
    stack = [(out[0] if strided else out).grad_fn]
    while stack:
        f = stack.pop()
        if f is None or f in names:
            continue
        names.add(f)
        stack.extend(q for q, _ in f.next_functions)
    names = {f.name() for f in names}
    want = {'fine_identity': '_MLPBlockBackward', 'fine_strided': '_MLPBlockBackward', 'coarse_identity': '_MLPSmallBackward',
            'coarse_grouped': '_MLPSmallGroupBackward'}[name]
    assert want in names, names
    assert ('_MLPBlockJoinBackward' if lv == 0 else '_MLPSmallJoinBackward') in names, names


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('name', ['fine_identity', 'coarse_grouped'])
def test_no_fold_without_the_callers_promise(name, mask_passes, monkeypatch):
    """The first block's output has a consumer outside the chain and the caller passes no input_mask: nothing folds (both mask passes
    run, the handshake stays open) and the gradients equal those of the switched-off path."""
    from crfconv_amd import ops
    chain = _chain(name)
    x = chain[4].clone().requires_grad_(True)
    monkeypatch.setattr(ops.state, 'no_mask_fold', False)
    del mask_passes[:]
    got = _run_chain(chain, x, wired=False, outside_consumer=True)
    assert len(mask_passes) == 2 and not got[3].folded and got[3].slope == pytest.approx(0.01)
    monkeypatch.setattr(ops.state, 'no_mask_fold', True)
    _assert_same(got, _run_chain(chain, x, wired=False, outside_consumer=True))


@pytest.mark.usefixtures('big_forms_from_4096')
@pytest.mark.parametrize('name', ['fine_strided', 'coarse_grouped'])
def test_two_block_chain_replayed_from_a_graph_equals_eager(name, monkeypatch):
    """Forward + backward of the wired chain captured once and replayed on two other inputs copied into the static buffer: the fold was
    decided while the capture issued the forward, replays need nothing from the host."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'no_mask_fold', False)
    chain = _chain(name)
    g = torch.Generator().manual_seed(31)
    xs = [torch.randn(chain[4].shape, generator=g).to(DEV) for _ in range(2)]
    x_static = chain[4].clone().requires_grad_(True)
    eager = []
    for xv in xs:
        x_static.data.copy_(xv)
        eager.append(_run_chain(chain, x_static))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run_chain(chain, x_static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    x_static.grad = None
    with torch.cuda.graph(graph):
        (blk_a, blk_b), geo_a, geo_b, strided, _, go, ga = chain
        for blk in (blk_a, blk_b):
            for p in blk.parameters():
                p.grad = None
        hs = ops.JoinMask()
        h = blk_a(x_static * 1.0, geo_a[0], geo_a[1], join_mask=hs)
        out, alias = blk_b(h, geo_b[0], geo_b[1], return_input_alias=True, input_mask=hs)
        torch.autograd.backward([out, alias * 0.5], [go, ga])
    assert hs.folded
    params = {'%d.%s' % (i, k): p for i, blk in enumerate((blk_a, blk_b)) for k, p in blk.named_parameters()}
    for i, xv in enumerate(xs):
        for blk in (blk_a, blk_b):
            for m in blk.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.reset_running_stats()
        x_static.data.copy_(xv)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same((out.detach(), x_static.grad, {k: p.grad for k, p in params.items()}, None), eager[i])
    assert int(ops.gridsync_ws(DEV).abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------------------- whole network

@pytest.mark.usefixtures('big_forms_from_4096')
def test_whole_network_fold_on_equals_fold_off(mask_passes, monkeypatch):
    """PointConvBig(6, 13, use_crf=True, steps=3), forward + loss + backward on two 4096-point clouds: equal logits, equal gradients
    (1e-6 on the atomics parameters), ONE mask pass (conv5_2's join, read by the decoder alone) instead of ten."""
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
    net = models.PointConvBig(6, 13, use_crf=True, steps=3)
    sd = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 5)
    net = net.to(DEV).train()
    y = torch.from_numpy(labels.reshape(-1)).long().to(DEV) - 1
    res, counts = {}, {}
    for fold in (True, False):
        monkeypatch.setattr(ops.state, 'no_mask_fold', not fold)
        net.load_state_dict(sd)                         # the same running statistics and dropout counter in both runs
        for p in net.parameters():
            p.grad = None
        del mask_passes[:]
        with train.no_autograph():
            logits = net(data)
            loss = torch.nn.functional.cross_entropy(logits, y, ignore_index=-1)
            loss.backward()
        counts[fold] = len(mask_passes)
        res[fold] = (logits.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert counts == {True: 1, False: 10}, counts
    assert torch.equal(res[True][0], res[False][0])
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) > 100
    for k, a in res[True][1].items():
        b = res[False][1][k]
        if 'point_conv' in k and 'weight_nn.1.lin' in k:
            assert_close(a, b, 1e-6, k)
        else:
            assert torch.equal(a, b), (k, float((a - b).abs().max()))
