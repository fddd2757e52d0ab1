"""blocks.BlockVotes restated in NumPy, on top of tests/sliding_blocks_restatement.py (imported as it is), and the inputs that
tests/test_host_block_votes.py and tests/test_gpu_block_votes.py share.

The definition.  A split of N points has R block rows; row r is point rows[r] and mask[r] says whether it lies in its block's un-padded
core.  np_reverse is the inverse table: per point its rows, ascending.  One update with scores [R', C] that cover rows
row_offset .. row_offset + R' takes, per point p, the rows of p in that range that pass `core` -- 'all': every row; 'only': mask == 1;
'prefer': mask == 1 if p has such a row ANYWHERE in the split, else every row -- in ascending order, forms
s = ((t_1 + t_2) + t_3) + .. with one rounding per add (t = the score, or exp of it), and then sums[p] = sums[p] + s, count[p] += rows used.
NpBlockVotes runs that in float32 (dtype=np.float32: the bits BlockVotes is held to where exp=False) or in float64 (the yardstick of the
bounds).  The adds run in an explicit loop over the position k inside a point's list -- the k-th row of every point that has one -- so
the order of every point's adds is the ascending row order; nothing is scattered with np.add.at.

brute_lists says the same with one scan of rows per point."""
import numpy as np

import _seeded as S
import sliding_blocks_restatement as R

CORE_MODES = ('all', 'only', 'prefer')
# the tests' own dense set: a point of a large scene lies in (floor(1.2 / 0.25) + 1)^2 = 25 blocks
DENSE = dict(block_size=1.0, stride=0.25, padding=0.1, min_points=1, proportion=0.02, count_form='ratio')


# ---------------------------------------------------------------------------------------------------------------- the definition
def np_reverse(rows, n_points):
    """(rev_ptr [N + 1] int64, rev_rows [R] int32): rev_rows[rev_ptr[p] : rev_ptr[p + 1]] = the r with rows[r] == p, ascending."""
    rows = np.asarray(rows, np.int64)
    order = np.argsort(rows, kind='stable')
    rev_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_points))]).astype(np.int64)
    return rev_ptr, order.astype(np.int32)


def brute_lists(rows, n_points):
    """[the r with rows[r] == p, ascending] per point, by one scan of rows per point."""
    rows = np.asarray(rows, np.int64)
    return [np.nonzero(rows == p)[0].tolist() for p in range(n_points)]


def row_use(split, n_points, core):
    """bool [R]: whether a row counts for its point under `core` (decided over the whole split)."""
    rows, mask = split['rows'], split['mask'] == 1
    if core == 'all':
        return np.ones(len(rows), bool)
    if core == 'only':
        return mask.copy()
    if core == 'prefer':
        has_core = np.zeros(n_points, bool)
        has_core[rows[mask]] = True
        return np.where(has_core[rows], mask, True)
    raise ValueError(core)


def used_lists(split, n_points, core, lo, hi):
    """The rows lo <= r < hi that count, grouped by point: (r, point, position in the point's list) per used row, and n [N] rows used."""
    r = np.arange(len(split['rows']))
    sel = r[row_use(split, n_points, core) & (r >= lo) & (r < hi)]
    sel = sel[np.argsort(split['rows'][sel], kind='stable')]                       # by point; ascending r inside a point
    pts = split['rows'][sel]
    n = np.bincount(pts, minlength=n_points).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    return sel, pts, np.arange(len(sel)) - start[pts], n


class NpBlockVotes:
    """BlockVotes in NumPy.  dtype=np.float32: every add rounds to float32; dtype=np.float64: terms (exp included) and sums in float64."""

    def __init__(self, split, n_points, num_classes, core='prefer', exp=False, dtype=np.float32):
        if core not in CORE_MODES:
            raise ValueError(core)
        self.split, self.n_points, self.C, self.core, self.exp, self.dtype = split, n_points, num_classes, core, exp, dtype
        self.sums = np.zeros((n_points, num_classes), dtype)
        self.count = np.zeros(n_points, np.int32)

    def update(self, scores, row_offset=0):
        scores = np.asarray(scores, np.float32)
        lo, hi = row_offset, row_offset + len(scores)
        assert 0 <= lo and hi <= self.split['n_rows'] and scores.shape[1:] == (self.C,)
        term = scores.astype(self.dtype)
        if self.exp:
            term = np.exp(term).astype(self.dtype)
        sel, pts, rank, n = used_lists(self.split, self.n_points, self.core, lo, hi)
        s = np.zeros((self.n_points, self.C), self.dtype)
        for k in range(int(rank.max()) + 1 if len(rank) else 0):                   # the k-th row of every point that has one
            at = rank == k
            p, t = pts[at], term[sel[at] - lo]                                     # (each point at most once: a plain assignment)
            s[p] = t if k == 0 else (s[p] + t).astype(self.dtype)
        hit = n > 0
        self.sums[hit] = (self.sums[hit] + s[hit]).astype(self.dtype)
        self.count += n.astype(np.int32)
        return n

    def result(self, reduce='mean', fill=-1):
        if reduce not in ('mean', 'sum'):
            raise ValueError(reduce)
        hit = self.count > 0
        out = np.zeros_like(self.sums)
        if reduce == 'sum':
            out[hit] = self.sums[hit]
        else:
            out[hit] = (self.sums[hit] / self.count[hit].astype(self.dtype)[:, None]).astype(self.dtype)
        pred = np.full(self.n_points, fill, np.int64)
        pred[hit] = np.argmax(self.sums[hit], axis=1)                              # the first maximum
        return out, pred

    def confusion(self, labels, label_shift=0, out=None):
        hist = np.zeros((self.C, self.C), np.int64) if out is None else out
        t = np.asarray(labels, np.int64) - label_shift
        pred = self.result('sum')[1]
        for p in np.nonzero((self.count > 0) & (t >= 0) & (t < self.C))[0]:
            hist[t[p], pred[p]] += 1
        return hist


def point_kinds(split, n_points):
    """(points without a row, with rows but no core row, with core rows and others) -- the three branches of 'prefer'."""
    n_all = np.bincount(split['rows'], minlength=n_points)
    n_core = np.bincount(split['rows'][split['mask'] == 1], minlength=n_points)
    return int((n_all == 0).sum()), int(((n_all > 0) & (n_core == 0)).sum()), int(((n_core > 0) & (n_core < n_all)).sum())


# ---------------------------------------------------------------------------------------------------------------- the inputs
def scores_for(seed, n_rows, C, log_probs=False):
    """Seeded scores [n_rows, C] float32.  Plain form: uniform in (-6, 2) -- negative values, sums that round at every add --, and where
    C >= 2 class 1 repeats class 0 raised by 1.5, so the two tie exactly at the top of many points: the first arg-max must answer 0.
    log_probs: a log-softmax, what the networks return (for exp=True)."""
    a = S.uniform(seed, 'scores', (n_rows, C), -6.0, 2.0)
    if log_probs:
        a64 = a.astype(np.float64)
        return (a64 - np.log(np.exp(a64).sum(1, keepdims=True))).astype(np.float32)
    if C >= 2:
        a[:, 0] = a[:, 0] + np.float32(1.5)
        a[:, 1] = a[:, 0]
    return a


def chunk_bounds(n_blocks):
    """Three uneven block ranges b0 .. b1 that cover the split."""
    a, b = n_blocks // 5, n_blocks // 5 + n_blocks // 2 + 1
    return [(0, a), (a, b), (b, n_blocks)]


def cases():
    """name -> (pos, ptr or None, parameter set): the splits the GPU test merges on."""
    parts = R.ragged_scenes()
    return {'yard': (R.yard_scene(), None, R.NPM3D), 'planar_dense': (R.planar_scene(), None, DENSE),
            'carved_small_dense': (R.carved_small_scene(), None, DENSE), 'tiny': (R.tiny_scene(), None, R.SCANNET),
            'ragged': (np.concatenate(parts), R.ptr_of(parts), R.SCANNET)}
