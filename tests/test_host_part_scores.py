"""The part IoU of ragged shape batches as far as it goes without a GPU: the fifth public header's prototypes, what ``utils.PartScores``
refuses before it reaches the library, the NumPy restatement (tests/part_scores_restatement.py) against the reference's recorded values and
the oracle, and the conditions on the inputs of tests/test_gpu_part_scores.py, so that test cannot hide behind its inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_counts import N_FUNCTIONS, N_RECORDS
import part_scores_restatement as R
from crfconv_amd import _lib
from oracle import eval_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_public_parts_header_declares_the_entries():
    with open(os.path.join(ROOT, 'include', 'crfconv_amd.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS          # (the first header's counts are pinned: its tables stay its own)
    with open(os.path.join(ROOT, 'include', 'crfconv_parts.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert functions == _lib.PARTS_SIGNATURES and records == {} and _lib.PARTS_RECORDS == {}
    assert sorted(functions) == ['crfconv_part_predict', 'crfconv_part_scores_update', 'crfconv_part_scores_workspace']
    for other in (_lib.SIGNATURES, _lib.INTERNAL_SIGNATURES, _lib.BLOCKS_SIGNATURES, _lib.VOTES_SIGNATURES, _lib.GRID_SIGNATURES):
        assert not set(functions) & set(other)
    v, i, l, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert functions['crfconv_part_scores_workspace'] == (z, [l, i])
    assert functions['crfconv_part_scores_update'] == (i, [v, v, v, l, i, v, v, l, v, v, i, i, v, z, v, v, v, v, v, v, v])
    assert functions['crfconv_part_predict'] == (i, [v, l, i, v, v, l, v, v, i, i, v, v])
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in functions)
    query = lib.crfconv_part_scores_workspace
    assert query(0, 50) == 0 and query(-1, 50) == 0 and query(5, 0) == 0 and query(5, 65) == 0 and query(1 << 31, 50) == 0
    assert query(1, 1) == 12 and query(20, 50) == 20 * 3 * 50 * 4 and query((1 << 31) - 1, 64) == ((1 << 31) - 1) * 3 * 64 * 4


def test_a_name_of_another_header_is_refused(tmp_path):
    clash = tmp_path / 'clash.h'
    clash.write_text('int crfconv_part_predict(int a);\n')
    with pytest.raises(_lib.CrfConvError, match='declares a name of another header again'):
        _lib._tables(str(clash), 'clash.h', (_lib.PARTS_SIGNATURES,))


def test_a_c_caller_sees_the_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
    assert cc is not None, 'no C compiler on PATH'
    src = tmp_path / 'caller.c'
    src.write_text('#include "crfconv_parts.h"\n'
                   'size_t (*query)(int64_t, int) = crfconv_part_scores_workspace;\n'
                   'int (*update)(const int64_t*, const int64_t*, const float*, int64_t, int, const int64_t*, const int64_t*, int64_t,\n'
                   '              const int32_t*, const int32_t*, int, int, void*, size_t, int64_t*, double*, int32_t*, float*, int32_t*,\n'
                   '              int32_t*, crf_stream_t) = crfconv_part_scores_update;\n'
                   'int (*predict)(const float*, int64_t, int, const int64_t*, const int64_t*, int64_t, const int32_t*, const int32_t*, int,\n'
                   '               int, int64_t*, crf_stream_t) = crfconv_part_predict;\n')
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'caller.o')])


# ----------------------------------------------------------------------------------------------------------------------- the refusals
@pytest.fixture
def never(monkeypatch):
    def reached(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', reached)
    monkeypatch.setattr(_lib, 'load', reached)


def test_the_table_is_checked(never):
    from crfconv_amd.utils import PartScores
    ps = PartScores.shapenet()
    assert ps.parts == R.SHAPENET_PARTS and ps.names == R.SHAPENET_NAMES and ps.n_labels == 50 and ps.n_cat == 16
    assert PartScores([[0, 2], [1]]).n_labels == 3 and PartScores([[0, 2], [1]]).names == ['0', '1']
    for parts, what in (([[0, 1], []], 'is empty'), ([[1, 0]], 'not ascending'), ([[0, 1, 1]], 'not ascending'),
                        ([[0, 50]], 'outside'), ([[-1, 3]], 'outside'), ([], 'categories'), ([[0]] * 65, 'categories'),
                        ([['a']], 'list of lists'), (7, 'list of lists')):
        with pytest.raises(ValueError, match=what):
            PartScores(parts, n_labels=50)
    for n_labels in (0, 65):
        with pytest.raises(ValueError, match='n_labels'):
            PartScores([[0]], n_labels=n_labels)
    with pytest.raises(ValueError, match='names'):
        PartScores([[0], [1]], names=['a'])
    with pytest.raises(ValueError, match='names'):
        PartScores([[0], [1]], names=['a', 'a'])
    with pytest.raises(ValueError, match='no CPU path'):
        PartScores([[0]], device='cpu')


def test_update_and_predict_refuse_bad_arguments_before_the_library(never):
    from crfconv_amd.utils import PartScores
    ps = PartScores.shapenet()
    N, S = 10, 2
    y, preds, scores = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64), torch.zeros((N, 50))
    ptr, cat = torch.tensor([0, 4, N]), torch.zeros(S, dtype=torch.int64)
    with pytest.raises(ValueError, match='exactly one of scores and preds'):
        ps.update(y, ptr, cat)
    with pytest.raises(ValueError, match='exactly one of scores and preds'):
        ps.update(y, ptr, cat, scores=scores, preds=preds)
    for bad in (y.int(), y.reshape(N, 1), y.float(), y.numpy()):
        with pytest.raises(ValueError, match=r'label_trues must be an int64 tensor \[N\]'):
            ps.update(bad, ptr, cat, preds=preds)
    for bad in (preds.int(), preds[:-1], preds.reshape(N, 1), preds.tolist()):
        with pytest.raises(ValueError, match='preds must be an int64 tensor'):
            ps.update(y, ptr, cat, preds=bad)
    for bad in (scores.double(), scores.half(), scores.reshape(-1), scores.reshape(N, 50, 1), scores.numpy()):
        with pytest.raises(ValueError, match='scores must be a float32 tensor'):
            ps.update(y, ptr, cat, scores=bad)
        with pytest.raises(ValueError, match='scores must be a float32 tensor'):
            ps.predict(bad, ptr, cat)
    for bad in (scores[:, :49], torch.zeros((N, 64))):
        with pytest.raises(ValueError, match='the part table has 50 labels'):
            ps.update(y, ptr, cat, scores=bad)
        with pytest.raises(ValueError, match='the part table has 50 labels'):
            ps.predict(bad, ptr, cat)
    with pytest.raises(ValueError, match='9 rows of scores for 10 labels'):
        ps.update(y, ptr, cat, scores=scores[:9])
    for bad in (ptr.int(), ptr.reshape(1, 3), torch.zeros(0, dtype=torch.int64), [0, 4, N]):
        with pytest.raises(ValueError, match=r'ptr must be an int64 tensor \[S \+ 1\]'):
            ps.update(y, bad, cat, preds=preds)
        with pytest.raises(ValueError, match=r'ptr must be an int64 tensor \[S \+ 1\]'):
            ps.predict(scores, bad, cat)
    for bad in (cat.int(), cat[:1], torch.zeros(3, dtype=torch.int64), cat.reshape(S, 1), [0, 0]):
        with pytest.raises(ValueError, match=r'category must be an int64 tensor \[S\]'):
            ps.update(y, ptr, bad, preds=preds)
        with pytest.raises(ValueError, match=r'category must be an int64 tensor \[S\]'):
            ps.predict(scores, ptr, bad)
    with pytest.raises(ValueError, match='ptr names no shape'):
        ps.update(y, torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), preds=preds)
    # everything else in order: only the device is missing
    with pytest.raises(ValueError, match='must be on the device'):
        ps.update(y, ptr, cat, preds=preds)
    with pytest.raises(ValueError, match='must be on the device'):
        ps.update(y, ptr, cat, scores=scores)
    with pytest.raises(ValueError, match='must be on the device'):
        ps.predict(scores, ptr, cat)
    # nothing was updated, so the state reads as zeros without a device
    assert not ps.category_IoU.any() and not ps.category_num.any() and ps.category_IoU.dtype == np.float32


# ------------------------------------------------------------------------------------------- the restatement against the reference
def test_restatement_reproduces_the_recorded_reference_values():
    case = R.fixture()
    g = case['g']
    ref = R.NpPartScores(case['parts'], case['names'], 50)
    out = ref.update(case['y'], case['ptr'], case['category'], preds=case['preds'])
    assert out['iou'].dtype == np.float64 and (out['iou'] == g['ious']).all()                 # ==, not a tolerance
    pIoU, mpIoU, table = ref.get_scores()
    assert pIoU == g['pIoU'] and np.isnan(mpIoU) and np.isnan(g['mpIoU'])
    cls = np.array([table[n] for n in g['cls_names']])
    assert np.array_equal(np.isnan(cls), np.isnan(g['cls'])) and (cls[~np.isnan(cls)] == g['cls'][~np.isnan(cls)]).all()
    assert ref.category_num.tolist() == np.bincount(g['cats'], minlength=16).tolist() and ref.bad == 0


@pytest.mark.parametrize('name', ['ragged', 'many'])
@pytest.mark.parametrize('mode', R.MODES)
def test_restatement_equals_the_oracle_shape_by_shape(name, mode):
    case = R.CASES[name]()
    out = R.NpPartScores(case['parts'], case['names'], case['C']).update(case['y'], case['ptr'], case['category'], **R.mode_args(case, mode))
    ptr = case['ptr']
    for s, c in enumerate(case['category']):
        sel = slice(ptr[s], ptr[s + 1])
        assert out['iou'][s] == eval_oracle.shapenet_part_iou(case['y'][sel], out['pred'][sel], case['parts'][c]), (s, c)
    assert (out['iou'][np.diff(ptr) == 0] == 1.0).all()                                        # an empty shape: exactly 1.0


def test_restricted_predictions_follow_the_sequential_rule():
    """np_predict against the contract's own words, row by row: start at the first part, replace only when strictly greater"""
    case = R.c64()
    scores, ptr = case['scores'], case['ptr']
    for restrict in (True, False):
        got = R.np_predict(scores, ptr, case['category'], case['parts'], restrict)
        for s, c in enumerate(case['category']):
            L = case['parts'][c] if restrict else list(range(64))
            for r in range(ptr[s], ptr[s + 1], 7):
                arg, best = L[0], scores[r, L[0]]
                for l in L[1:]:
                    if scores[r, l] > best:
                        arg, best = l, scores[r, l]
                assert got[r] == arg
    first = np.repeat([case['parts'][c][0] for c in case['category']], np.diff(ptr))
    stuck = np.isnan(scores[np.arange(len(first)), first])
    assert stuck.sum() >= 100 and (R.np_predict(scores, ptr, case['category'], case['parts'])[stuck] == first[stuck]).all()


# ------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
def _tied(case):
    """per row: whether the maximum among the parts of its shape's category is reached more than once"""
    tied = np.zeros(len(case['y']), bool)
    for s, c in enumerate(case['category']):
        sub = case['scores'][case['ptr'][s]:case['ptr'][s + 1]][:, case['parts'][c]]
        tied[case['ptr'][s]:case['ptr'][s + 1]] = (sub == sub.max(axis=1, keepdims=True)).sum(axis=1) > 1
    return tied


@pytest.mark.parametrize('name', ['ragged', 'many'])
def test_scores_have_ties_and_the_restriction_matters(name):
    case = R.CASES[name]()
    scores, N = case['scores'], len(case['y'])
    assert scores.shape == (N, 50) and scores.dtype == np.float32 and (scores * 2 == np.round(scores * 2)).all()
    assert -4.0 <= scores.min() and scores.max() < 7.0
    own = R.np_predict(scores, case['ptr'], case['category'], case['parts'], True)
    free = R.np_predict(scores, case['ptr'], case['category'], case['parts'], False)
    print('%s: restricted != unrestricted on %.2f of the rows, tied maximum on %.3f' % (name, (own != free).mean(), _tied(case).mean()))
    assert (own != free).mean() >= 0.5 and _tied(case).mean() >= 0.05
    assert ((case['preds'] < 0) | (case['preds'] >= 50)).sum() >= 0.005 * N                    # predictions that match no part
    inside = np.concatenate([np.isin(case['y'][case['ptr'][s]:case['ptr'][s + 1]], case['parts'][c]) for s, c in enumerate(case['category'])])
    assert 0.85 < inside.mean() < 0.97                                                         # and labels of another category's parts


@pytest.mark.parametrize('name', ['ragged', 'many'])
def test_the_float32_steps_differ_from_one_rounding(name):
    case = R.CASES[name]()
    differ = {}
    for mode in R.MODES:
        ref = R.NpPartScores(case['parts'], case['names'], 50)
        out = ref.update(case['y'], case['ptr'], case['category'], **R.mode_args(case, mode))
        once = R.double_sum_rounded_once(out['iou'], case['category'], 16)
        differ[mode] = int((ref.category_IoU.view(np.uint32) != once.view(np.uint32)).sum())
        print('%s / %s: %d categories differ from the double sum rounded once' % (name, mode, differ[mode]))
    # the default mode (scores, restricted) of each case shows it; ragged adds twice onto three categories only, so not every mode does
    assert differ['restrict'] >= 1 and sum(differ.values()) >= 2


def test_many_has_a_window_that_meets_eight_shapes():
    case = R.many()
    sizes = np.diff(case['ptr'])
    assert len(sizes) == 300 and sizes.min() == 0 and sizes.max() == 40 and set(case['category'].tolist()) == set(range(16))
    N = len(case['y'])
    best = 0
    for r0 in range(0, N, R.TILE):                         # the tiles of the count pass themselves, which are narrower than 256 rows
        owners = np.searchsorted(case['ptr'], np.arange(r0, min(r0 + R.TILE, N)), side='right')
        best = max(best, len(set(owners.tolist())))
    assert best >= 8 and R.TILE <= 256
    assert np.bincount(case['category'], minlength=16).min() >= 8                             # many float32-step adds per category


def test_ragged_has_the_sizes():
    case = R.ragged()
    sizes = np.diff(case['ptr']).tolist()
    assert sizes == R.RAGGED_SIZES and len(case['y']) == 21811 and case['category'].tolist() == list(range(16)) + [4, 4, 15, 0]
    assert max(sizes) >= 4 * R.TILE and R.TILE <= 1024
    assert sizes[0] == 0 and sizes[11] == 0 and sizes[10:20][1] == 0                           # first, interior, first-but-one of a second chunk
    assert (case['ptr'][1:-1] % R.TILE != 0).sum() >= 15                                       # borders inside tiles
    assert {63, 65, 1, 2}.issubset(sizes)


def test_c64_and_bad_are_what_they_say():
    case = R.c64()
    assert case['C'] == 64 and len(case['parts']) == 4 and any(len(L) == 1 for L in case['parts']) and any(63 in L for L in case['parts'])
    assert case['scores'].shape[1] == 64 and np.isnan(case['scores']).sum() >= 150
    assert (R.np_predict(case['scores'], case['ptr'], case['category'], case['parts']) == 63).sum() > 50
    case, good = R.bad(), R.ragged()
    assert (case['category'] != good['category']).sum() == 2 and sorted(case['category'][[3, 7]].tolist()) == [-1, 16]
    ref = R.NpPartScores(case['parts'], case['names'], 50)
    out = ref.update(case['y'], case['ptr'], case['category'], scores=case['scores'])
    assert np.isnan(out['iou']).nonzero()[0].tolist() == [3, 7] and ref.bad == 2 and ref.category_num.sum() == 18
    assert (out['pred'][case['ptr'][3]:case['ptr'][4]] == -1).all() and not out['counts'][[3, 7]].any()
