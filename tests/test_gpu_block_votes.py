"""crfconv_amd.blocks.BlockVotes on the GPU against the NumPy restatement (tests/block_votes_restatement.py): the inverse table exactly,
sums / count / result bit for bit where the terms are the scores themselves, against float64 within a derived bound where they are
expf(score), chunked updates through BlockSplit.select, repeated updates, empty inputs, determinism, the confusion matrix through the
existing entry, call counts, one captured update and the argument checks.  tests/test_host_block_votes.py holds the conditions on these
inputs."""
import numpy as np
import pytest
import torch

import _seeded as S
import block_votes_restatement as V
import sliding_blocks_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24                    # unit roundoff of float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope='module')
def splits():
    """name -> dict(n, want: the restated split, got: the device BlockSplit, pos, ptr); nothing here is written again (the device
    split caches its inverse table, which is the point)."""
    from crfconv_amd import blocks
    out = {}
    for name, (pos, ptr, prm) in V.cases().items():
        out[name] = dict(n=len(pos), want=R.np_sliding_blocks(pos, ptr, **prm), pos=pos, ptr=ptr, prm=prm,
                         got=blocks.sliding_blocks(dev(pos), None if ptr is None else dev(ptr), **prm))
    return out


@pytest.fixture(scope='module')
def references():
    """(case, C, core, exp, dtype, chunks) -> the restatement's votes after those updates, computed once."""
    memo = {}

    def get(case, C, core, exp=False, dtype=np.float32, chunks=None, times=1):
        key = (case['name'], C, core, exp, dtype, None if chunks is None else tuple(chunks), times)
        if key not in memo:
            votes = V.NpBlockVotes(case['want'], case['n'], C, core, exp, dtype)
            scores = V.scores_for(3400 + C, case['want']['n_rows'], C, log_probs=exp)
            for _ in range(times):
                for lo, hi in chunks or [(0, len(scores))]:
                    votes.update(scores[lo:hi], lo)
            memo[key] = votes
        return memo[key]
    return get


@pytest.fixture(scope='module')
def case(splits):
    def get(name):
        return dict(splits[name], name=name)
    return get


@pytest.fixture
def calls(monkeypatch):
    """Names of the library calls made through _lib.call while the fixture is live."""
    from crfconv_amd import _lib
    seen = []
    real = _lib.call

    def call(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


def check_reverse(split, want, n, what):
    rev_ptr, rev_rows = split.reverse()
    want_ptr, want_rows = V.np_reverse(want['rows'], n)
    assert rev_ptr.is_cuda and rev_ptr.dtype == torch.int64 and rev_rows.dtype == torch.int32, what
    assert np.array_equal(rev_ptr.cpu().numpy(), want_ptr) and np.array_equal(rev_rows.cpu().numpy(), want_rows), what


@pytest.mark.parametrize('params', ['scannet', 'loose', 'dense'])
@pytest.mark.parametrize('scene', sorted(R.SCENES))
def test_reverse_equals_the_restatement(scene, params, calls):
    from crfconv_amd import blocks
    prm = V.DENSE if params == 'dense' else R.PARAM_SETS[params]
    p = R.SCENES[scene]()
    split = blocks.sliding_blocks(dev(p), **prm)
    check_reverse(split, R.np_sliding_blocks(p, **prm), len(p), (scene, params))
    del calls[:]
    again = split.reverse()
    assert calls == [] and again[0] is split.reverse()[0] and again[1] is split.reverse()[1]


@pytest.mark.parametrize('params', ['scannet', 'loose', 'dense'])
def test_reverse_of_the_ragged_batch(params):
    from crfconv_amd import blocks
    prm = V.DENSE if params == 'dense' else R.PARAM_SETS[params]
    parts = R.ragged_scenes()
    pos, ptr = np.concatenate(parts), R.ptr_of(parts)
    check_reverse(blocks.sliding_blocks(dev(pos), dev(ptr), **prm), R.np_sliding_blocks(pos, ptr, **prm), len(pos), params)


@pytest.mark.parametrize('core', V.CORE_MODES)
@pytest.mark.parametrize('C', [1, 5, 13, 50, 64])
@pytest.mark.parametrize('name', ['yard', 'planar_dense', 'ragged'])
def test_plain_sums_are_bit_identical(case, references, name, C, core):
    """exp=False: the term is read as it is, the sums use only additions in the stated order and the mean is one correctly rounded
    division, so every bit is fixed by the definition."""
    from crfconv_amd import blocks
    c = case(name)
    want = references(c, C, core)
    votes = blocks.BlockVotes(c['got'], C, core=core)
    votes.update(dev(V.scores_for(3400 + C, c['want']['n_rows'], C)))
    assert votes.sums.dtype == torch.float32 and votes.count.dtype == torch.int32 and tuple(votes.sums.shape) == (c['n'], C)
    assert np.array_equal(votes.count.cpu().numpy(), want.count)
    assert np.array_equal(bits(votes.sums), bits(want.sums))
    for reduce, fill in (('mean', -1), ('sum', -7)):
        out, pred = votes.result(reduce, fill=fill)
        want_out, want_pred = want.result(reduce, fill=fill)
        assert out.dtype == torch.float32 and pred.dtype == torch.int64
        assert np.array_equal(bits(out), bits(want_out)), reduce
        assert np.array_equal(pred.cpu().numpy(), want_pred), reduce
    if name != 'planar_dense':
        assert (want_pred == -7).sum() >= 469                                      # the fill is exercised


@pytest.mark.parametrize('core', ['prefer', 'all'])
@pytest.mark.parametrize('C', [5, 20])
@pytest.mark.parametrize('name', ['yard', 'planar_dense'])
def test_exp_sums_against_float64(case, references, name, C, core):
    """exp=True.  Per element |got - want| <= (n_p + 3) 2^-24 S, n_p the rows used for the point and S the float64 sum of its terms
    (all positive, so every partial sum is at most S).  In units of u S, u = 2^-24: the expf terms 2 -- HIP's math API reference lists
    expf at a maximum error of 1 ulp (the table of single precision mathematical functions in the HIP C++ language extensions; the
    documentation installed with ROCm holds the runtime API index only and not that table, so it is cited by name), and 1 ulp of a
    term is at most 2 u of it --, the n_p - 1 sequential roundings one each, the add onto sums one, and half of one for comparing in
    float64 what the device holds in float32: n_p + 2.5, rounded up to n_p + 3.  'mean': the same divided by n_p, plus one rounding of
    the quotient."""
    from crfconv_amd import blocks
    c = case(name)
    want = references(c, C, core, exp=True, dtype=np.float64)
    votes = blocks.BlockVotes(c['got'], C, core=core, exp=True)
    votes.update(dev(V.scores_for(3400 + C, c['want']['n_rows'], C, log_probs=True)))
    n = want.count.astype(np.float64)[:, None]
    assert np.array_equal(votes.count.cpu().numpy(), want.count)
    got = votes.sums.cpu().numpy()
    assert got.dtype == np.float32 and (got[want.count == 0] == 0).all()
    err, bound = np.abs(got.astype(np.float64) - want.sums), (n + 3) * U * want.sums
    print('exp sums: largest error / bound = %.3f' % float((err[want.count > 0] / bound[want.count > 0]).max()))
    assert (err <= bound).all()
    hit = want.count > 0
    for reduce in ('mean', 'sum'):
        out, pred = votes.result(reduce, fill=-2)
        out = out.cpu().numpy().astype(np.float64)
        want_out = want.result(reduce)[0]
        lim = bound if reduce == 'sum' else bound / np.maximum(n, 1) + U * (want_out + bound / np.maximum(n, 1))
        assert (np.abs(out - want_out) <= lim).all() and (out[~hit] == 0).all(), reduce
        pred = pred.cpu().numpy()
        assert np.array_equal(pred[hit], np.argmax(got[hit], axis=1)) and (pred[~hit] == -2).all()


@pytest.mark.parametrize('core', V.CORE_MODES)
@pytest.mark.parametrize('name', ['yard', 'planar_dense', 'ragged'])
def test_chunked_updates_through_select(case, references, name, core):
    """Three uneven block ranges through BlockSplit.select: the bits of the restatement run with the same chunks, and within
    2 (n_p - 1) 2^-24 S of the one-shot run -- each is within (n_p - 1) u S of the exact sum (n_p - 1 roundings in either: a chunk of
    n_j rows makes n_j - 1, and the add of a partial sum onto sums one more, except onto the zeros of the first).  The scores are signed
    here, so S is the sum of their magnitudes."""
    from crfconv_amd import blocks
    from crfconv_amd.data import Data
    c, C = case(name), 13
    split, want_split = c['got'], c['want']
    scores = V.scores_for(3400 + C, want_split['n_rows'], C)
    d_scores = dev(scores)
    pos_block, x = split.features('room')
    chunks = V.chunk_bounds(want_split['n_blocks'])
    row_chunks = [(int(want_split['ptr'][b0]), int(want_split['ptr'][b1])) for b0, b1 in chunks]
    votes = blocks.BlockVotes(split, C, core=core)
    for (b0, b1), (r0, r1) in zip(chunks, row_chunks):
        data, row_offset = split.select(b0, b1, x, split.rows)
        assert isinstance(data, Data) and row_offset == r0 and isinstance(row_offset, int)
        assert np.array_equal(data.ptr.cpu().numpy(), want_split['ptr'][b0:b1 + 1] - r0) and data.ptr.dtype == torch.int64
        assert np.array_equal(data.batch.cpu().numpy(), want_split['batch'][r0:r1] - b0)
        assert torch.equal(data.pos, pos_block[r0:r1]) and torch.equal(data.x, x[r0:r1]) and torch.equal(data.y, split.rows[r0:r1])
        assert np.array_equal(data.mask.cpu().numpy(), want_split['mask'][r0:r1])
        assert np.array_equal(data.indices.cpu().numpy(), want_split['indices'][r0:r1])
        votes.update(d_scores[r0:r1], row_offset)                                  # (the network's scores of the chunk)
    want = references(c, C, core, chunks=row_chunks)
    assert np.array_equal(votes.count.cpu().numpy(), want.count) and np.array_equal(bits(votes.sums), bits(want.sums))
    whole = references(c, C, core)
    assert np.array_equal(whole.count, want.count)
    S_abs = V.NpBlockVotes(want_split, c['n'], C, core, dtype=np.float64)
    S_abs.update(np.abs(scores))
    bound = 2 * (want.count.astype(np.float64)[:, None] - 1).clip(min=0) * U * S_abs.sums
    assert (np.abs(votes.sums.cpu().numpy().astype(np.float64) - whole.sums.astype(np.float64)) <= bound).all()
    assert (bits(want.sums) != bits(whole.sums)).any()                             # (the chunks do change the order of the adds)


def test_select_checks_its_arguments(case):
    c = case('yard')
    split = c['got']
    x = split.features('room')[1]
    for b0, b1 in ((-1, 2), (3, 2), (0, split.n_blocks + 1)):
        with pytest.raises(ValueError):
            split.select(b0, b1, x)
    with pytest.raises(ValueError):
        split.select(0, 1, x[:-1])
    with pytest.raises(ValueError):
        split.select(0, 1, x, split.rows[:-1])
    data, r0 = split.select(2, 2, x)                                               # an empty range of blocks
    assert r0 == int(c['want']['ptr'][2]) and data.x.shape[0] == 0 and data.ptr.tolist() == [0] and data.y is None


@pytest.mark.parametrize('name', ['yard', 'planar_dense'])
def test_two_updates_add_up(case, references, name):
    from crfconv_amd import blocks
    c, C = case(name), 5
    want = references(c, C, 'prefer', times=2)
    votes = blocks.BlockVotes(c['got'], C)
    d_scores = dev(V.scores_for(3400 + C, c['want']['n_rows'], C))
    votes.update(d_scores)
    once = votes.count.clone()
    votes.update(d_scores)
    assert np.array_equal(bits(votes.sums), bits(want.sums)) and torch.equal(votes.count, 2 * once)
    assert np.array_equal(votes.count.cpu().numpy(), want.count)
    votes.reset()
    assert not votes.sums.any() and not votes.count.any()
    votes.update(d_scores)
    assert np.array_equal(bits(votes.sums), bits(references(c, C, 'prefer').sums))


def test_empty_inputs(case, calls):
    from crfconv_amd import blocks
    c = case('tiny')
    assert c['got'].n_blocks == 0
    rev_ptr, rev_rows = c['got'].reverse()
    assert rev_ptr.tolist() == [0] * (c['n'] + 1) and tuple(rev_rows.shape) == (0,) and rev_rows.dtype == torch.int32
    votes = blocks.BlockVotes(c['got'], 7, exp=True)
    votes.update(torch.zeros((0, 7), dtype=torch.float32, device=DEV))
    out, pred = votes.result('mean', fill=-5)
    torch.cuda.synchronize()
    assert (pred == -5).all() and not votes.count.any() and not out.any() and tuple(out.shape) == (c['n'], 7)
    hist = votes.confusion(dev(np.zeros(c['n'], np.int64)))
    assert not hist.any()                                                          # 300 labels of class 0, no point covered: nothing counted
    assert 'crfconv_block_reverse' not in calls and 'crfconv_block_votes_update' not in calls
    # no point at all
    none = blocks.sliding_blocks(torch.zeros((0, 3), dtype=torch.float32, device=DEV), **R.SCANNET)
    votes = blocks.BlockVotes(none, 3)
    votes.update(torch.zeros((0, 3), dtype=torch.float32, device=DEV))
    out, pred = votes.result()
    assert tuple(out.shape) == (0, 3) and tuple(pred.shape) == (0,) and not votes.confusion(torch.zeros(0, dtype=torch.int64, device=DEV)).any()
    # a batch with an empty scene in front and one in the middle
    parts = [np.zeros((0, 3), np.float32), R.carved_scene(), np.zeros((0, 3), np.float32), R.strip_scene() + np.float32(9.0)]
    pos, ptr = np.concatenate(parts), R.ptr_of(parts)
    want_split = R.np_sliding_blocks(pos, ptr, **R.SCANNET)
    split = blocks.sliding_blocks(dev(pos), dev(ptr), **R.SCANNET)
    check_reverse(split, want_split, len(pos), 'empty scenes')
    scores = V.scores_for(3450, want_split['n_rows'], 4)
    want = V.NpBlockVotes(want_split, len(pos), 4)
    want.update(scores)
    votes = blocks.BlockVotes(split, 4)
    votes.update(dev(scores))
    assert np.array_equal(bits(votes.sums), bits(want.sums)) and np.array_equal(votes.count.cpu().numpy(), want.count)


def test_two_runs_are_bit_identical_and_a_scene_does_not_see_its_batch(case):
    from crfconv_amd import blocks
    c, C = case('ragged'), 20
    scores = V.scores_for(3460, c['want']['n_rows'], C, log_probs=True)
    runs = []
    for _ in range(2):
        split = blocks.sliding_blocks(dev(c['pos']), dev(c['ptr']), **c['prm'])     # a fresh split: a fresh inverse table
        votes = blocks.BlockVotes(split, C, exp=True)
        votes.update(dev(scores))
        runs.append([t.clone() for t in split.reverse()] + [votes.sums.clone(), votes.count.clone()] + list(votes.result('mean')))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # scene 5 (about 4300 points) alone, with the scores of its own rows
    s = 5
    lo, hi = int(c['ptr'][s]), int(c['ptr'][s + 1])
    mine = np.nonzero(c['want']['scene'] == s)[0]
    r0, r1 = int(c['want']['ptr'][mine[0]]), int(c['want']['ptr'][mine[-1] + 1])
    alone = blocks.sliding_blocks(dev(c['pos'][lo:hi]), **c['prm'])
    assert alone.n_rows == r1 - r0 > 10000
    votes = blocks.BlockVotes(alone, C, exp=True)
    votes.update(dev(scores[r0:r1]))
    assert torch.equal(votes.sums.view(torch.int32), runs[0][2][lo:hi].view(torch.int32)) and torch.equal(votes.count, runs[0][3][lo:hi])


@pytest.mark.parametrize('name', ['yard', 'ragged'])
def test_confusion_equals_the_restatement(case, references, name):
    from crfconv_amd import blocks
    from crfconv_amd.utils.metrics import iou_from_confusions
    c, C = case(name), 13
    want = references(c, C, 'prefer')
    votes = blocks.BlockVotes(c['got'], C)
    votes.update(dev(V.scores_for(3400 + C, c['want']['n_rows'], C)))
    labels = S.integers(3470, 'labels', (c['n'],), -1, C + 1)                        # -1 and C are outside: skipped
    hist = votes.confusion(dev(labels))
    want_hist = want.confusion(labels)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (C, C) and np.array_equal(hist.cpu().numpy(), want_hist)
    covered = want.count > 0
    assert int(hist.sum()) == int((covered & (labels >= 0) & (labels < C)).sum()) < int(((labels >= 0) & (labels < C)).sum())
    # uncovered points contribute nothing, whatever their labels say (class 0 is where an all-zero row would land)
    moved = np.where(covered, labels, 0)
    assert np.array_equal(votes.confusion(dev(moved)).cpu().numpy(), want_hist)
    out = hist.clone()
    assert votes.confusion(dev(labels + 1), label_shift=1, out=out) is out and np.array_equal(out.cpu().numpy(), 2 * want_hist)
    assert iou_from_confusions(hist.cpu().numpy()).shape == (C,)
    with pytest.raises(ValueError):
        votes.confusion(dev(labels[:-1]))
    with pytest.raises(ValueError):
        votes.confusion(dev(labels), out=torch.zeros((C, C), dtype=torch.int32, device=DEV))


def test_calls_do_not_grow_with_the_blocks(case, calls):
    from crfconv_amd import blocks
    seen = {}
    for name in ('yard', 'planar_dense'):
        c = case(name)
        c['got'].reverse()
        votes = blocks.BlockVotes(c['got'], 9)
        d_scores = dev(V.scores_for(3480, c['want']['n_rows'], 9))
        del calls[:]
        votes.update(d_scores)
        upd = list(calls)
        del calls[:]
        votes.result()
        seen[name] = (c['got'].n_blocks, upd, list(calls))
    assert seen['planar_dense'][0] > 8 * seen['yard'][0]
    for name in seen:
        assert seen[name][1] == ['crfconv_block_votes_update'] and seen[name][2] == ['crfconv_block_votes_result']


def test_a_captured_update_replays(case, references):
    from crfconv_amd import blocks
    c, C = case('yard'), 5
    votes = blocks.BlockVotes(c['got'], C)
    d_scores = dev(V.scores_for(3400 + C, c['want']['n_rows'], C))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        votes.update(d_scores)                                                     # the warm-up: the first of three updates
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        votes.update(d_scores)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want = references(c, C, 'prefer', times=3)
    assert np.array_equal(bits(votes.sums), bits(want.sums)) and np.array_equal(votes.count.cpu().numpy(), want.count)


def test_argument_checks(case):
    from crfconv_amd import blocks
    c = case('yard')
    split, n_rows = c['got'], c['want']['n_rows']
    for C in (0, 65):
        with pytest.raises(ValueError):
            blocks.BlockVotes(split, C)
    with pytest.raises(ValueError):
        blocks.BlockVotes(split, 5, core='centre')
    with pytest.raises(ValueError):
        blocks.BlockVotes(c['want'], 5)                                            # not a BlockSplit
    votes = blocks.BlockVotes(split, 5)
    good = torch.zeros((n_rows, 5), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        votes.update(good.cpu())
    with pytest.raises(ValueError):
        votes.update(good[:, :4])                                                  # a wrong C
    with pytest.raises(ValueError):
        votes.update(good.double())
    with pytest.raises(ValueError):
        votes.update(good.reshape(-1))
    for part, off in ((good, 1), (good[:10], n_rows - 9), (good[:10], -1)):
        with pytest.raises(ValueError):
            votes.update(part, off)
    votes.update(good[:10], n_rows - 10)                                           # the last ten rows: allowed
    votes.update(good[:, :5].t().contiguous().t())                                 # not contiguous: taken as its contiguous copy
    with pytest.raises(ValueError):
        votes.result('median')
    with pytest.raises(ValueError):
        votes.confusion(torch.zeros(c['n'] + 1, dtype=torch.int64, device=DEV))
    assert not votes.sums.any()                                                    # (zeros were added)
