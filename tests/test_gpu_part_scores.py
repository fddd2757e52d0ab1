"""-m gpu: ``crfconv_amd.utils.PartScores`` (csrc/part_scores.hip) against the NumPy restatement (tests/part_scores_restatement.py) and
the reference's recorded values, bit for bit in every output: predictions, counts, the float64 per-shape IoU and the float32 running
state.  The inputs and the conditions on them are checked without a GPU in tests/test_host_part_scores.py."""
import numpy as np
import pytest
import torch

import part_scores_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    """device tensor against array: dtype, shape and bits (NaN included)"""
    got = host(got) if torch.is_tensor(got) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    view = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(got.dtype)
    return np.array_equal(got.view(view), want.view(view)) if view else np.array_equal(got, want)


def new_scores(case):
    from crfconv_amd.utils import PartScores
    return PartScores(case['parts'], names=case['names'], n_labels=case['C'], device=DEV)


def same_state(ps, ref):
    return same_bits(ps.category_IoU, ref.category_IoU) and same_bits(ps.category_num, ref.category_num)


@pytest.fixture(scope='module')
def cases():
    """name -> the case with its device tensors under 'd'; nothing here is written again"""
    out = {}
    for name, make in R.CASES.items():
        case = make()
        case['d'] = {k: dev(case[k]) for k in ('y', 'preds', 'scores', 'ptr', 'category')}
        out[name] = case
    return out


@pytest.fixture(scope='module')
def references(cases):
    """(name, mode, times) -> (the restatement's state after `times` updates with the whole batch, the last update's outputs), once each"""
    memo = {}

    def get(name, mode, times=1):
        if (name, mode, times) not in memo:
            case = cases[name]
            ref = R.NpPartScores(case['parts'], case['names'], case['C'])
            for _ in range(times):
                out = ref.update(case['y'], case['ptr'], case['category'], **R.mode_args(case, mode))
            memo[name, mode, times] = (ref, out)
        return memo[name, mode, times]
    return get


def d_args(case, mode):
    d = case['d']
    return dict(preds=d['preds']) if mode == 'preds' else dict(scores=d['scores'], restrict=mode == 'restrict')


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


def test_the_fixture_as_one_call(cases, references):
    case = cases['fixture']
    g, d = case['g'], case['d']
    ref, want = references('fixture', 'preds')
    ps = new_scores(case)
    assert ps.parts == type(ps).shapenet(DEV).parts and ps.names == type(ps).shapenet(DEV).names
    iou = ps.update(d['y'], d['ptr'], d['category'], preds=d['preds'])
    assert iou.dtype == torch.float64 and iou.device == torch.device(DEV) and same_bits(iou, g['ious']) and same_bits(iou, want['iou'])
    assert same_state(ps, ref)
    pIoU, mpIoU, table = ps.get_scores()
    assert pIoU == g['pIoU'] and np.isnan(mpIoU) and np.isnan(g['mpIoU']) and list(table) == g['cls_names'].tolist()
    cls = np.array([table[n] for n in g['cls_names']])
    assert np.array_equal(np.isnan(cls), np.isnan(g['cls'])) and (cls[~np.isnan(cls)] == g['cls'][~np.isnan(cls)]).all()


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', ['ragged', 'many', 'c64'])
def test_a_batch_equals_the_restatement(cases, references, name, mode):
    case = cases[name]
    d = case['d']
    ref, want = references(name, mode)
    ps = new_scores(case)
    iou, counts, pred = ps.update(d['y'], d['ptr'], d['category'], return_counts=True, return_preds=True, **d_args(case, mode))
    assert counts.dtype == torch.int32 and same_bits(counts, want['counts'])
    assert same_bits(iou, want['iou']) and not np.isnan(want['iou']).any()
    assert pred.dtype == torch.int64 and same_bits(pred, want['pred'])
    assert same_state(ps, ref)
    # without the extras the counters live in the workspace: the same values
    ps.reset()
    assert same_bits(ps.update(d['y'], d['ptr'], d['category'], **d_args(case, mode)), want['iou']) and same_state(ps, ref)
    if mode != 'preds':
        alone = ps.predict(d['scores'], d['ptr'], d['category'], restrict=mode == 'restrict')
        assert alone.dtype == torch.int64 and same_bits(alone, want['pred'])
        assert same_state(ps, ref)                                                             # (predict leaves the state alone)


def test_chunked_updates_equal_the_one_call(cases, references):
    case = cases['ragged']
    d, ptr = case['d'], case['ptr']
    ref, want = references('ragged', 'restrict')
    ps = new_scores(case)
    got = []
    for s0, s1 in ((0, 10), (10, 20)):
        r0, r1 = int(ptr[s0]), int(ptr[s1])
        got.append(ps.update(d['y'][r0:r1], d['ptr'][s0:s1 + 1] - r0, d['category'][s0:s1], scores=d['scores'][r0:r1]))
    assert same_bits(torch.cat(got), want['iou']) and same_state(ps, ref)
    # twice the same batch
    twice, _ = references('ragged', 'restrict', times=2)
    ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])
    assert same_state(ps, twice) and (twice.category_num == 2 * ref.category_num).all()
    assert (twice.category_IoU.view(np.uint32) != ref.category_IoU.view(np.uint32)).sum() == 16
    ps.reset()
    assert not ps.category_IoU.any() and not ps.category_num.any()
    ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])
    assert same_state(ps, ref)


def test_five_runs_give_the_same_bits(cases, references):
    case = cases['many']
    d = case['d']
    ref, want = references('many', 'restrict')
    for _ in range(5):
        ps = new_scores(case)
        iou, counts, pred = ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'], return_counts=True, return_preds=True)
        assert same_bits(iou, want['iou']) and same_bits(counts, want['counts']) and same_bits(pred, want['pred']) and same_state(ps, ref)


def test_bad_shapes_get_nan_and_are_counted(cases, references):
    case = cases['bad']
    d = case['d']
    ref, want = references('bad', 'restrict')
    good = references('ragged', 'restrict')[1]
    ps = new_scores(case)
    iou, counts, pred = ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'], return_counts=True, return_preds=True)
    got = host(iou)
    assert np.isnan(got).nonzero()[0].tolist() == [3, 7] and same_bits(iou, want['iou'])
    keep = np.ones(20, bool)
    keep[[3, 7]] = False
    assert np.array_equal(got[keep].view(np.uint64), good['iou'][keep].view(np.uint64))        # every other shape as in `ragged`
    assert same_bits(counts, want['counts']) and same_bits(pred, want['pred'])
    with pytest.raises(ValueError, match='2 shapes'):
        ps.get_scores()
    with pytest.raises(ValueError, match='2 shapes'):
        ps.category_IoU
    _, _, cat_sum, cat_num, n_bad = ps._state
    assert same_bits(cat_sum, ref.category_IoU) and same_bits(cat_num, ref.category_num) and int(n_bad) == ref.bad == 2
    ps.reset()
    assert ps.get_scores()[2].keys() == dict.fromkeys(case['names']).keys() and not ps.category_num.any()
    # bounds outside the batch: NaN and counted, and the rows before them are scored as ever
    cut = d['ptr'].clone()
    cut[-1] += 5
    iou = host(ps.update(d['y'], cut, cases['ragged']['d']['category'], preds=d['preds']))
    assert np.isnan(iou[19]) and same_bits(iou[:19], references('ragged', 'preds')[1]['iou'][:19])
    with pytest.raises(ValueError, match='1 shapes'):
        ps.category_num


def test_update_and_predict_read_nothing_back(cases, calls):
    case = cases['ragged']
    d = case['d']
    ps = new_scores(case)
    ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])                             # (the table and the workspace are made here)
    del calls[:]
    ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])
    ps.update(d['y'], d['ptr'], d['category'], preds=d['preds'], return_counts=True)
    ps.predict(d['scores'], d['ptr'], d['category'])
    assert calls == ['crfconv_part_scores_workspace', 'crfconv_part_scores_update', 'crfconv_part_scores_update', 'crfconv_part_predict']


def test_a_captured_update_replays(cases, references):
    case = cases['ragged']
    d = case['d']
    ps = new_scores(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])                         # the warm-up: the first of three updates
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iou = ps.update(d['y'], d['ptr'], d['category'], scores=d['scores'])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    ref, want = references('ragged', 'restrict', times=3)
    assert same_bits(iou, want['iou']) and same_state(ps, ref) and (ref.category_num.sum() == 60)


def test_views_of_scores_are_copied_and_other_dtypes_refused(cases, references):
    """scores that are not contiguous are taken as their contiguous copy; scores that are not float32 are refused"""
    case = cases['c64']
    d = case['d']
    ref, want = references('c64', 'restrict')
    wide = torch.zeros((len(case['y']), 80), dtype=torch.float32, device=DEV)
    wide[:, 7:71] = d['scores']
    view = wide[:, 7:71]
    assert not view.is_contiguous()
    ps = new_scores(case)
    assert same_bits(ps.update(d['y'], d['ptr'], d['category'], scores=view), want['iou']) and same_state(ps, ref)
    assert same_bits(ps.predict(d['scores'].t().contiguous().t(), d['ptr'], d['category']), want['pred'])
    # rows that start 4 bytes off a 16-byte border: the copy to LDS goes word by word, the values are the same
    flat = torch.zeros(d['scores'].numel() + 1, dtype=torch.float32, device=DEV)
    off = flat[1:].view(-1, 64)
    off.copy_(d['scores'])
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert same_bits(ps.predict(off, d['ptr'], d['category']), want['pred'])
    for bad in (d['scores'].double(), d['scores'].half()):
        with pytest.raises(ValueError, match='scores must be a float32 tensor'):
            ps.update(d['y'], d['ptr'], d['category'], scores=bad)
    assert same_state(ps, ref)


def test_empty_batches(cases):
    case = cases['ragged']
    ps = new_scores(case)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    iou = ps.update(none, torch.zeros(4, dtype=torch.int64, device=DEV), dev(np.array([2, 2, 5], np.int64)), preds=none)
    assert host(iou).tolist() == [1.0, 1.0, 1.0] and ps.category_num.tolist()[2] == 2 and ps.category_IoU[2] == 2.0
    iou = ps.update(none, torch.zeros(1, dtype=torch.int64, device=DEV), none, scores=torch.zeros((0, 50), device=DEV))
    assert tuple(iou.shape) == (0,) and ps.category_num.sum() == 3
