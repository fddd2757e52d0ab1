"""Farthest point sampling restated in float64 numpy, and the inputs that tests/test_host_fps.py and tests/test_gpu_fps.py share.

np_fps is the definition: pick t + 1 is the argmax, ties to the lower index as numpy.argmax gives, of every point's smallest squared
distance to picks 0 ... t.  It also reports, per pick, by how much the winner beat the runner-up (relative to the winner): a float32
kernel can only be held to the SAME picks where that margin is far above float32 rounding.  walk_along checks picks in pick order
without asking for the same picks: each must be a farthest point within `tol`."""
import numpy as np

import _seeded as S

TOL = 1e-5          # about 100 float32 roundings of a three-term squared distance; a wrong pick misses by far more

# the ragged batch: R = 1, 2, 3, 5 and 8 rows per thread, a one-point cloud, a cloud below a wavefront, one past a multiple of 1024
SIZES = [700, 300, 9, 2048, 40, 1, 1025, 4097, 8192]
RATIO = 0.25
EXACT = [700, 300, 9, 40, 1, 1025]           # clouds of the batch whose every margin is above TOL (asserted by the host test)

# (seed, n, ratio) of the single clouds of the other tiers whose margins are above TOL
TIER_CASES = [(950, 16448, 96), (951, 40960, 64)]


def ragged_clouds():
    """The float32 clouds of the ragged batch, each in its own place."""
    return [(S.make_cloud(900 + s, n, box=(2, 1, 1)) + np.float32(3.0 * s)).astype(np.float32) for s, n in enumerate(SIZES)]


def n_picks(n, ratio):
    import math
    if n == 0:
        return 0
    return max(1, math.ceil(ratio * n)) if isinstance(ratio, float) else min(ratio, n)


def np_fps(p, m, first=0):
    """(picks [m] in pick order, smallest relative margin between a winner and its runner-up; inf without a contest)."""
    p = np.asarray(p, dtype=np.float64)
    d = np.full(len(p), np.inf)
    picks, margin = [first], np.inf
    for _ in range(m - 1):
        d = np.minimum(d, ((p - p[picks[-1]]) ** 2).sum(1))
        cur = int(np.argmax(d))
        if len(p) > 1 and d[cur] > 0:
            second = np.partition(d, -2)[-2]
            margin = min(margin, (d[cur] - second) / d[cur])
        elif len(p) > 1:
            margin = 0.0
        picks.append(cur)
    return np.array(picks, dtype=np.int64), margin


def walk_along(p, picks, tol=TOL):
    """Smallest, over the picks after the first, of (the pick's distance to the picks before it) / (the largest such distance in the
    cloud); asserts it is at least 1 - tol."""
    p = np.asarray(p, dtype=np.float64)
    d = np.full(len(p), np.inf)
    worst = 1.0
    for t in range(len(picks) - 1):
        d = np.minimum(d, ((p - p[picks[t]]) ** 2).sum(1))
        far = d.max()
        if far > 0:
            worst = min(worst, d[picks[t + 1]] / far)
        assert d[picks[t + 1]] >= (1 - tol) * far, (t, picks[t + 1], d[picks[t + 1]], far)
    return worst
