"""blocks.BlockVotes as far as it goes without a GPU: the NumPy restatement (tests/block_votes_restatement.py) against one scan of rows
per point and plain Python sums, the third public header's prototypes, and the conditions on the inputs of
tests/test_gpu_block_votes.py -- all three branches of 'prefer' fire, points lie in as many blocks as the parameters allow, one split is
empty, the ragged batch has uncovered points, a chunk boundary cuts a point's list -- so that test cannot hide behind its fixtures."""
import ctypes
import os

import numpy as np
import pytest

import block_votes_restatement as V
import sliding_blocks_restatement as R
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def splits():
    """name -> (number of points, the restated split); nothing here is written again."""
    return {name: (len(pos), R.np_sliding_blocks(pos, ptr, **prm)) for name, (pos, ptr, prm) in V.cases().items()}


@pytest.fixture(scope='module')
def lists(splits):
    return {name: V.brute_lists(splits[name][1]['rows'], splits[name][0]) for name in ('yard', 'planar_dense')}


# ------------------------------------------------------------------------------------------------ the restatement is the definition
@pytest.mark.parametrize('name', ['yard', 'planar_dense'])
def test_reverse_is_the_scan_of_rows_per_point(splits, lists, name):
    n, split = splits[name]
    rev_ptr, rev_rows = V.np_reverse(split['rows'], n)
    assert rev_ptr.dtype == np.int64 and rev_rows.dtype == np.int32 and rev_ptr.shape == (n + 1,) and rev_rows.shape == (split['n_rows'],)
    assert rev_ptr[0] == 0 and rev_ptr[-1] == split['n_rows']
    for p in range(n):
        assert rev_rows[rev_ptr[p]:rev_ptr[p + 1]].tolist() == lists[name][p], p


def plain_votes(split, rows_of, n, C, core, exp, scores, chunks, dtype):
    """sums, count by Python loops: per update and point, its rows filtered and added one after the other."""
    sums, count = np.zeros((n, C), dtype), np.zeros(n, np.int32)
    for lo, hi in chunks:
        for p in range(n):
            mine = rows_of[p]
            has_core = any(split['mask'][r] == 1 for r in mine)
            only_core = core == 'only' or (core == 'prefer' and has_core)
            s, used = None, 0
            for r in mine:
                if not lo <= r < hi or (only_core and split['mask'][r] != 1):
                    continue
                t = scores[r].astype(dtype)
                t = np.exp(t).astype(dtype) if exp else t
                s = t if s is None else (s + t).astype(dtype)
                used += 1
            if used:
                sums[p] = (sums[p] + s).astype(dtype)
                count[p] += used
    return sums, count


@pytest.mark.parametrize('name,exp,dtype', [('yard', False, np.float32), ('yard', True, np.float64), ('planar_dense', False, np.float32)])
@pytest.mark.parametrize('core', V.CORE_MODES)
def test_restatement_is_the_definition(splits, lists, name, core, exp, dtype):
    n, split = splits[name]
    C = 3
    scores = V.scores_for(3401, split['n_rows'], C, log_probs=exp)
    cut = split['n_rows'] // 3 + 1
    for chunks in ([(0, split['n_rows'])], [(0, cut), (cut, split['n_rows'])]):
        votes = V.NpBlockVotes(split, n, C, core, exp, dtype)
        for lo, hi in chunks:
            votes.update(scores[lo:hi], lo)
        sums, count = plain_votes(split, lists[name], n, C, core, exp, scores, chunks, dtype)
        assert votes.sums.dtype == dtype and np.array_equal(votes.sums, sums) and np.array_equal(votes.count, count)
    out, pred = votes.result('mean', fill=-3)
    hit = count > 0
    assert (pred[~hit] == -3).all() and (out[~hit] == 0).all()
    assert pred[hit].tolist() == [max(range(C), key=lambda c: (row[c], -c)) for row in sums[hit]]
    assert np.array_equal(out[hit], (sums[hit] / count[hit].astype(dtype)[:, None]).astype(dtype))
    assert np.array_equal(votes.result('sum')[0], np.where(hit[:, None], sums, 0))
    labels = np.arange(n) % (C + 1)                          # class C is outside: skipped
    hist = votes.confusion(labels)
    want = np.zeros((C, C), np.int64)
    for p in range(n):
        if hit[p] and labels[p] < C:
            want[labels[p], pred[p]] += 1
    assert np.array_equal(hist, want) and hist.sum() == int((hit & (labels < C)).sum())
    assert np.array_equal(votes.confusion(labels + 1, label_shift=1, out=hist.copy()), 2 * want)


def test_scores_have_negative_values_and_exact_ties(splits):
    n, split = splits['yard']
    for C in (5, 13):
        scores = V.scores_for(3402, split['n_rows'], C)
        assert scores.dtype == np.float32 and (scores < 0).mean() > 0.5 and np.array_equal(scores[:, 0], scores[:, 1])
        votes = V.NpBlockVotes(split, n, C, 'prefer')
        votes.update(scores)
        top = votes.sums.max(1)
        tied = (votes.count > 0) & (votes.sums[:, 0] == top) & (votes.sums[:, 1] == top)
        assert tied.sum() > 1000 and (votes.result()[1][tied] == 0).all()          # (a last arg-max would answer 1 there)
    logp = V.scores_for(3402, split['n_rows'], 9, log_probs=True)
    assert (logp < 0).all() and np.allclose(np.exp(logp.astype(np.float64)).sum(1), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ the header
def test_the_public_votes_header_declares_the_entries():
    with open(os.path.join(ROOT, 'include', 'crfconv_block_votes.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert functions == _lib.VOTES_SIGNATURES and records == {} and _lib.VOTES_RECORDS == {}
    assert sorted(functions) == ['crfconv_block_reverse', 'crfconv_block_reverse_workspace', 'crfconv_block_votes_result',
                                 'crfconv_block_votes_update']
    others = set(_lib.SIGNATURES) | set(_lib.INTERNAL_SIGNATURES) | set(_lib.BLOCKS_SIGNATURES)
    assert not set(functions) & others
    v, i, l, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert functions['crfconv_block_reverse_workspace'] == (z, [l, l])
    assert functions['crfconv_block_reverse'] == (i, [v, l, l, v, v, z, v, v, v])
    assert functions['crfconv_block_votes_update'] == (i, [v, l, l, i, v, v, l, l, i, i, v, v, v])
    assert functions['crfconv_block_votes_result'] == (i, [v, v, l, i, i, l, v, v, v])
    lib = _lib.load()
    for name, (res, args) in functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert 'crfconv_vote_confusion' in _lib.SIGNATURES                             # (the confusion goes through the existing entry)


def test_the_module_has_the_modes():
    from crfconv_amd import blocks
    assert blocks.CORE_MODES == {'all': 0, 'only': 1, 'prefer': 2} and blocks.REDUCE_FORMS == {'sum': 0, 'mean': 1}
    assert blocks.MAX_CLASSES == 64 and blocks.MAX_MEMBERSHIPS == 64
    assert all(hasattr(blocks.BlockVotes, m) for m in ('update', 'result', 'confusion', 'reset'))
    assert all(hasattr(blocks.BlockSplit, m) for m in ('reverse', 'select'))


def test_the_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                                # never read: every call below is refused by its argument checks
    assert lib.crfconv_block_reverse_workspace(0, 5) == 0 and lib.crfconv_block_reverse_workspace(5, 0) == 0
    assert lib.crfconv_block_reverse_workspace(5, 1 << 31) == 0 and lib.crfconv_block_reverse_workspace(100, 5000) > 5000 * 24
    assert lib.crfconv_block_reverse(None, 5, 5, one, one, 1 << 20, one, one, None) < 0
    assert lib.crfconv_block_reverse(one, 5, 5, one, one, 16, one, one, None) < 0              # workspace too small
    for C in (0, 65):
        assert lib.crfconv_block_votes_update(one, 5, 0, C, one, one, 5, 5, 0, 0, one, one, None) < 0
        assert lib.crfconv_block_votes_result(one, one, 5, C, 0, -1, one, one, None) < 0
    assert lib.crfconv_block_votes_update(one, 5, 1, 4, one, one, 5, 5, 0, 0, one, one, None) < 0      # rows 1 .. 6 of 5
    assert lib.crfconv_block_votes_update(one, 5, -1, 4, one, one, 5, 5, 0, 0, one, one, None) < 0
    assert lib.crfconv_block_votes_update(one, 5, 0, 4, one, one, 5, 5, 3, 0, one, one, None) < 0      # core
    assert lib.crfconv_block_votes_update(one, 5, 0, 4, one, one, 5, 5, 0, 2, one, one, None) < 0      # use_exp
    assert lib.crfconv_block_votes_result(one, one, 5, 4, 2, -1, one, one, None) < 0                   # reduce
    assert 'reduce' in _lib.last_error()


# ------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
def test_yard_fires_all_three_branches_of_prefer(splits):
    n, split = splits['yard']
    assert n == 9000 and V.point_kinds(split, n) == (1048, 330, 2516)
    use = {core: V.row_use(split, n, core) for core in V.CORE_MODES}
    assert use['all'].all() and 0 < use['only'].sum() < use['prefer'].sum() < use['all'].sum()


def test_dense_scenes_fill_the_multiplicity(splits):
    assert R.max_multiplicity(**V.DENSE) == 25
    for name in ('planar_dense', 'carved_small_dense'):
        n, split = splits[name]
        assert R.multiplicity(split, n).max() == 25 and split['n_rows'] <= 72000 and n <= 10300
    n, split = splits['planar_dense']
    assert (split['n_blocks'], split['n_rows']) == (80, 37837)


def test_tiny_has_no_block_and_the_ragged_batch_uncovered_points(splits):
    n, split = splits['tiny']
    assert (split['n_blocks'], split['n_rows']) == (0, 0) and n == 300
    n, split = splits['ragged']
    sizes = [len(p) for p in R.ragged_scenes()]
    assert sizes[:5] == [0, 1, 63, 65, 1025] and sizes[6:] == [300, 4540] and 4100 <= sizes[5] <= 4100 + R.SORT_CHUNK
    assert V.point_kinds(split, n)[0] == 469 and n == sum(sizes) <= 10300


@pytest.mark.parametrize('name', ['yard', 'planar_dense', 'ragged'])
def test_chunk_boundaries_cut_a_list(splits, name):
    n, split = splits[name]
    chunks = V.chunk_bounds(split['n_blocks'])
    assert chunks[0][0] == 0 and chunks[-1][1] == split['n_blocks'] and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert len({b1 - b0 for b0, b1 in chunks}) == 3 and all(b1 > b0 for b0, b1 in chunks)
    rev_ptr, rev_rows = V.np_reverse(split['rows'], n)
    first, last = rev_rows[rev_ptr[:-1].clip(max=split['n_rows'] - 1)], rev_rows[(rev_ptr[1:] - 1).clip(min=0)]
    has = rev_ptr[1:] > rev_ptr[:-1]
    cuts = [int((has & (first < split['ptr'][b0]) & (last >= split['ptr'][b0])).sum()) for b0, _ in chunks[1:]]
    assert cuts[0] >= 1                                      # (the ragged batch's second boundary falls between two scenes: it cuts none)
    assert all(n >= 1 for n in cuts) or name == 'ragged'
