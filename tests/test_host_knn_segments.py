"""The segmented kNN's workspace is sized from (n_segments, total_pts) alone -- the split exists on the device only -- by a bound over
every split (csrc/knn.hip: seg_cells_bound).  crfconv_knn_segments_need is the layout arithmetic for ONE given split; here the bound
is held against it on random and extreme splits.  No GPU."""
import ctypes

import numpy as np
import pytest

from crfconv_amd import _lib


def need(sizes):
    arr = (ctypes.c_int64 * len(sizes))(*[int(v) for v in sizes])
    return _lib.load().crfconv_knn_segments_need(arr, len(sizes))


def grant(sizes):
    return _lib.load().crfconv_knn_segments_dev_workspace(len(sizes), int(sum(sizes)), 0, 16)


@pytest.mark.parametrize('total', [1, 100, 8192, 131072])
def test_workspace_bound_holds_for_every_split(total):
    rng = np.random.default_rng(total)
    splits = [[total], [1] * total if total <= 200 else [total - 199] + [1] * 199,            # one segment; one point per segment
              [0] * 199 + [total], [0] * 100 + [total] + [0] * 99, [total // 2, 0, 0, total - total // 2]]      # many empty segments
    while len(splits) < 1000:
        S = int(rng.integers(1, 201))
        kind = len(splits) % 3
        if kind == 0:                                        # cut points uniform over the rows: sizes of every scale, some empty
            cuts = np.sort(rng.integers(0, total + 1, S - 1))
            sizes = np.diff(np.concatenate([[0], cuts, [total]]))
        elif kind == 1:                                      # most segments tiny, a few large
            w = rng.random(S) ** 8
            sizes = np.floor(w / w.sum() * total).astype(np.int64)
            sizes[int(rng.integers(0, S))] += total - sizes.sum()
        else:                                                # as even as it gets: the sizes that maximise the sum of a concave need
            sizes = np.full(S, total // S, np.int64)
            sizes[: total % S] += 1
        assert sizes.sum() == total and (sizes >= 0).all()
        splits.append(sizes.tolist())
    worst = 0.0
    for sizes in splits:
        n, g = need(sizes), grant(sizes)
        assert 0 < n <= g, (sizes[:8], len(sizes), n, g)
        worst = max(worst, n / g)
    assert worst > 0.25                                      # the bound is not vacuous: some split uses a good part of it


def test_need_of_a_segment_matches_the_grid_rule():
    """0.6 points per cell: a cloud of n points has the largest g with 0.6 g^3 <= n cells per axis (at least 1, at most 160), and
    (g + 1)^3 cells; the int32 arrays per cell are what `need` grows by."""
    def cells(n):
        g = 1
        while g < 160 and 3 * (g + 1) ** 3 <= 5 * n:
            g += 1
        return (g + 1) ** 3
    for n in (0, 1, 4, 5, 16, 17, 75, 8192, 131072, 10 ** 7):
        assert cells(n) <= 8 + 4 * n
    # the per-cell part of the layout is three int32 arrays (256-byte aligned each): doubling the cells shows it
    a, b = need([8192]), need([8192, 8192])
    assert b - a >= 3 * 4 * cells(8192) and b - a <= 3 * 4 * cells(8192) + 8192 * 20 + 8 * 256
