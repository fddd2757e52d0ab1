"""The part IoU of a ragged batch of shapes, restated with NumPy from the contract in include/crfconv_parts.h: what
``crfconv_amd.utils.PartScores`` must return bit for bit -- predictions, the I / T / P counts, the per-shape IoU in float64 and the running
float32 category sums with one rounding per shape -- and the input cases of tests/test_gpu_part_scores.py with the conditions on them
(tests/test_host_part_scores.py checks those, and this restatement against the reference's values, without a GPU)."""
import os

import numpy as np

import _seeded as S

EPS = 2.0 ** -23
TILE = 128                        # rows per workgroup of the count pass (csrc/part_scores.hip)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g11_shapenet_score.npz')

SHAPENET_NAMES = ['Airplane', 'Bag', 'Cap', 'Car', 'Chair', 'Earphone', 'Guitar', 'Knife', 'Lamp', 'Laptop', 'Motorbike', 'Mug', 'Pistol',
                  'Rocket', 'Skateboard', 'Table']
SHAPENET_PARTS = [[0, 1, 2, 3], [4, 5], [6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18], [19, 20, 21], [22, 23], [24, 25, 26, 27],
                  [28, 29], [30, 31, 32, 33, 34, 35], [36, 37], [38, 39, 40], [41, 42, 43], [44, 45, 46], [47, 48, 49]]
# four categories over 64 labels: one with a single part, one that holds label 63, one wide and sparse
C64_PARTS = [[0, 1, 2, 5, 8, 13, 21, 34], [10], list(range(20, 50, 3)), [50, 57, 63]]

RAGGED_SIZES = [0, 1, 2, 63, 65, 257, 4097, 700, 2048, 2048, 1, 0, 3000, 129, 511, 1025, 2500, 64, 5000, 300]
RAGGED_CATEGORIES = list(range(16)) + [4, 4, 15, 0]


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def _valid(ptr, category, s, n_cat, N):
    return 0 <= category[s] < n_cat and 0 <= ptr[s] <= ptr[s + 1] <= N


def np_first_argmax(sub):
    """[n, k] -> [n]: the first column is the start value and a later one replaces it only when strictly greater."""
    start_nan = np.isnan(sub[:, 0])
    arg = np.where(np.isnan(sub), -np.inf, sub).argmax(axis=1)
    return np.where(start_nan, 0, arg)


def np_predict(scores, ptr, category, parts, restrict=True):
    """int64 [N]: -1 for a row of no shape and, restricted, for the rows of a shape whose category is outside the table."""
    N, pred = len(scores), np.full(len(scores), -1, np.int64)
    for s in range(len(ptr) - 1):
        lo, hi = max(int(ptr[s]), 0), min(int(ptr[s + 1]), N)
        if lo >= hi:
            continue
        if not restrict:
            pred[lo:hi] = np_first_argmax(scores[lo:hi])
        elif 0 <= category[s] < len(parts):
            L = np.asarray(parts[int(category[s])])
            pred[lo:hi] = L[np_first_argmax(scores[lo:hi][:, L])]
    return pred


def np_counts(y_true, y_pred, ptr, category, parts, C):
    """int32 [S, 3, C]: rows with t == l and p == l, with t == l, with p == l, for the labels l of the shape's list; zero elsewhere."""
    S_, N = len(ptr) - 1, len(y_true)
    out = np.zeros((S_, 3, C), np.int32)
    for s in range(S_):
        if not _valid(ptr, category, s, len(parts), N):
            continue
        t, p = y_true[ptr[s]:ptr[s + 1]], y_pred[ptr[s]:ptr[s + 1]]
        for l in parts[int(category[s])]:
            out[s, 0, l] = np.count_nonzero((t == l) & (p == l))
            out[s, 1, l] = np.count_nonzero(t == l)
            out[s, 2, l] = np.count_nonzero(p == l)
    return out


def np_shape_iou(counts, ptr, category, parts, N):
    """float64 [S] from the three counts: the sum starts at 0.0 and runs in list order; NaN for a bad shape."""
    out = np.full(len(category), np.nan, np.float64)
    for s in range(len(category)):
        if not _valid(ptr, category, s, len(parts), N):
            continue
        L = parts[int(category[s])]
        iu = 0.0
        for l in L:
            i, t, p = (int(v) for v in counts[s, :, l])
            iu = iu + (float(i) + EPS) / (float(t + p - i) + EPS)
        out[s] = iu / float(len(L))
    return out


class NpPartScores:
    """The running state: float32 category sums that take one shape at a time, one rounding each."""

    def __init__(self, parts, names=None, n_labels=None):
        self.parts = parts
        self.names = names or ['%d' % c for c in range(len(parts))]
        self.C = n_labels or 1 + max(l for L in parts for l in L)
        self.reset()

    def reset(self):
        self.category_IoU = np.zeros(len(self.parts), np.float32)
        self.category_num = np.zeros(len(self.parts), np.int32)
        self.bad = 0

    def update(self, y_true, ptr, category, scores=None, preds=None, restrict=True):
        """-> dict(iou, counts, pred)"""
        pred = np.asarray(preds, np.int64) if scores is None else np_predict(scores, ptr, category, self.parts, restrict)
        counts = np_counts(y_true, pred, ptr, category, self.parts, self.C)
        iou = np_shape_iou(counts, ptr, category, self.parts, len(y_true))
        for s, iu in enumerate(iou):
            if np.isnan(iu):
                self.bad += 1
                continue
            c = int(category[s])
            self.category_IoU[c] = np.float32(np.float64(self.category_IoU[c]) + iu)
            self.category_num[c] += 1
        return dict(iou=iou, counts=counts, pred=pred)

    def get_scores(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            per_class = self.category_IoU / self.category_num
            pIoU = self.category_IoU.sum() / self.category_num.sum()
        return pIoU, per_class.mean(), dict(zip(self.names, per_class))


def double_sum_rounded_once(iou, category, n_cat):
    """what the state would be if the shapes were summed in float64 and rounded at the end: NOT the contract (the host test shows it differs)"""
    out = np.zeros(n_cat, np.float64)
    for s, iu in enumerate(iou):
        if not np.isnan(iu):
            out[int(category[s])] += iu
    return out.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------- cases
def _labels(seed, sizes, category, parts, C):
    """y_true: nine rows in ten carry a part of their shape's category, the others any label; preds: the truth on 70 % of the rows, any
    label on the others, and a few values outside [0, C)."""
    ptr, rng = ptr_of(sizes), S._rng(seed, 'labels')
    N = int(ptr[-1])
    y = rng.integers(0, C, N)
    for s, c in enumerate(category):
        L = np.asarray(parts[c % len(parts)])
        own = L[rng.integers(0, len(L), sizes[s])]
        y[ptr[s]:ptr[s + 1]] = np.where(rng.random(sizes[s]) < 0.9, own, y[ptr[s]:ptr[s + 1]])
    preds = np.where(rng.random(N) < 0.7, y, rng.integers(0, C, N))
    outside = rng.random(N) < 0.01
    preds = np.where(outside, rng.choice([-1, C, C + 27, -(1 << 40)], N), preds)
    return y.astype(np.int64), preds.astype(np.int64)


def _scores(seed, y, C):
    """uniform in [-4, 4), rounded to multiples of 0.5 so that ties occur; on 60 % of the rows +3 on the true column"""
    rng = S._rng(seed, 'scores')
    scores = (np.floor(rng.uniform(-4.0, 4.0, (len(y), C)) * 2.0) / 2.0).astype(np.float32)
    lift = rng.random(len(y)) < 0.6
    scores[np.flatnonzero(lift), y[lift]] += np.float32(3.0)
    return scores


def _case(seed, sizes, category, parts, names, C):
    y, preds = _labels(seed, sizes, category, parts, C)
    return dict(y=y, preds=preds, scores=_scores(seed, y, C), ptr=ptr_of(sizes), category=np.asarray(category, np.int64), parts=parts,
                names=names, C=C)


def ragged():
    return _case(3600, RAGGED_SIZES, RAGGED_CATEGORIES, SHAPENET_PARTS, SHAPENET_NAMES, 50)


def many():
    """300 shapes of 0-40 rows with random categories: a tile spans many shapes and a category takes many float32-step adds"""
    rng = S._rng(3601, 'many')
    return _case(3601, rng.integers(0, 41, 300).tolist(), rng.integers(0, 16, 300).tolist(), SHAPENET_PARTS, SHAPENET_NAMES, 50)


def c64():
    """C = 64; some rows hold NaN scores, among them in the column of their category's first part (which then stays the prediction)"""
    sizes, category = [300, 5, 129, 1000, 64, 0, 77, 513], [0, 1, 2, 3, 1, 2, 3, 0]
    case = _case(3602, sizes, category, C64_PARTS, None, 64)
    rng = S._rng(3602, 'nan')
    rows = rng.permutation(len(case['y']))[:200]
    case['scores'][rows[:100], rng.integers(0, 64, 100)] = np.nan
    first = np.repeat([C64_PARTS[c][0] for c in category], sizes)
    case['scores'][rows[100:], first[rows[100:]]] = np.nan
    return case


def fixture():
    """the eight shapes of tests/golden/g11_shapenet_score.npz as one batch, with the reference's values for it"""
    g = np.load(GOLDEN)
    n = len(g['cats'])
    y = np.concatenate([g['yt%d' % i] for i in range(n)]).astype(np.int64)
    preds = np.concatenate([g['yp%d' % i] for i in range(n)]).astype(np.int64)
    return dict(y=y, preds=preds, scores=None, ptr=ptr_of([len(g['yt%d' % i]) for i in range(n)]), category=g['cats'].astype(np.int64),
                parts=SHAPENET_PARTS, names=SHAPENET_NAMES, C=50, g=g)


def bad():
    """``ragged`` with one category above the table and one below"""
    case = ragged()
    case['category'] = case['category'].copy()
    case['category'][3], case['category'][7] = 16, -1
    return case


CASES = {'ragged': ragged, 'many': many, 'c64': c64, 'fixture': fixture, 'bad': bad}
MODES = ('preds', 'restrict', 'all')


def mode_args(case, mode):
    """the keyword arguments of one of the three modes: preds, scores restricted to the category's parts, scores over all columns"""
    if mode == 'preds':
        return dict(preds=case['preds'])
    return dict(scores=case['scores'], restrict=mode == 'restrict')
