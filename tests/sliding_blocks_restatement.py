"""The sliding block split of a scene restated in NumPy, and the inputs that tests/test_host_sliding_blocks.py and
tests/test_gpu_sliding_blocks.py share.

np_sliding_blocks is the definition crfconv_amd.blocks.sliding_blocks is held to, bit for bit.  Per scene: a = pos - min(pos) in float32,
limit = max(a); block counts per axis in Python floats (float64) from float(limit); block (i, j) begins at (i * stride, j * stride) in
float64; (a minimum that is a zero of both signs counts as -0.0;) a point is in the block iff np.float32(beg - padding) <= a <= np.float32((beg + block_size) + padding) on x and y, compared in
float32, and in its core (mask) iff np.float32(beg) <= a <= np.float32(beg + block_size); a block is kept iff count >= min_points and
float(mask count) / float(count) >= proportion; kept blocks are numbered scene-major, then i, then j, and their rows ascend.  Every
float32 / float64 step is written out (np.float32(bound), float(limit)), so nothing hangs on a NumPy version's scalar promotion.

brute_sliding_blocks says the same with a Python loop over all cells and all points and no array operation at all.
"""
import math

import numpy as np

import _seeded as S

# the reference's four parameter sets (its dataset constructors) ...
SCANNET = dict(block_size=1.5, stride=1.0, padding=0.2, min_points=200, proportion=0.02, count_form='ratio')
S3DIS = dict(block_size=1.0, stride=0.5, padding=0.1, min_points=100, proportion=0.02, count_form='ratio')
SEMANTIC3D = dict(block_size=5.0, stride=3.0, padding=0.5, min_points=500, proportion=0.02, count_form='ceil_first')
NPM3D = dict(block_size=5.0, stride=3.0, padding=0.5, min_points=500, proportion=0.02, count_form='ceil_first')
REFERENCE_SETS = {'scannet': SCANNET, 's3dis': S3DIS, 'semantic3d': SEMANTIC3D, 'npm3d': NPM3D}
# ... and three of the tests' own: dyadic numbers, whose bounds the lattice scene meets exactly; the S3DIS geometry with the other count
# form, under which the 0.3 m scene has one candidate block; and a set that keeps the blocks of a handful of points
DYADIC = dict(block_size=1.5, stride=1.0, padding=0.25, min_points=50, proportion=0.02, count_form='ratio')
SMALL_CEIL = dict(block_size=1.0, stride=0.5, padding=0.1, min_points=100, proportion=0.02, count_form='ceil_first')
LOOSE = dict(block_size=1.0, stride=0.5, padding=0.1, min_points=1, proportion=0.02, count_form='ratio')
PARAM_SETS = dict(REFERENCE_SETS, dyadic=DYADIC, small_ceil=SMALL_CEIL, loose=LOOSE)

SORT_CHUNK = 1024          # rows per chunk of the library's radix sort (csrc/radix_sort.hpp)


# ---------------------------------------------------------------------------------------------------------------- the definition
def axis_blocks(limit32, block_size, stride, count_form):
    """Blocks along an axis whose float32 extent is limit32; the arithmetic is Python's (float64)."""
    lim = float(limit32)
    if count_form == 'ratio':
        c = int(math.ceil((lim - block_size) / stride)) + 1
    elif count_form == 'ceil_first':
        c = int(math.ceil(lim - block_size) / stride) + 1
    else:
        raise ValueError(count_form)
    return max(c, 0)


def block_bounds(i, block_size, stride, padding):
    """(padded low, padded high, core low, core high) of blocks i along an axis, float32, from float64 in the stated operation order."""
    beg = float(i) * float(stride)
    return (np.float32(beg - padding), np.float32((beg + block_size) + padding), np.float32(beg), np.float32(beg + block_size))


def align(p):
    """(a, pos_min, limit) of one scene's float32 points; zeros for an empty scene."""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if len(p) == 0:
        return p.copy(), np.zeros(3, np.float32), np.zeros(3, np.float32)
    pos_min = p.min(0)
    pos_min[((p == 0) & np.signbit(p)).any(0) & (pos_min == 0)] = np.float32(-0.0)      # a minimum of zeros of both signs: -0.0, whatever the order
    a = (p - pos_min).astype(np.float32)
    return a, pos_min, a.max(0)


def np_sliding_blocks(pos, ptr=None, *, block_size, stride, padding, min_points=200, proportion=0.02, count_form='ratio'):
    """dict of ptr, indices, rows, mask, batch, scene, cell, pos_min, limit, n_blocks, n_rows, as BlockSplit holds them, and for the
    tests' conditions: cells (candidate blocks), dropped_min_points, dropped_proportion, on_bound (rows that sit exactly on a padded
    bound of their block)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    ptr = np.array([0, len(pos)], np.int64) if ptr is None else np.asarray(ptr, dtype=np.int64)
    n_scenes = len(ptr) - 1
    out_ptr, indices, rows, mask, batch, scene, cell = [0], [], [], [], [], [], []
    pos_min, limit = np.zeros((n_scenes, 3), np.float32), np.zeros((n_scenes, 3), np.float32)
    cells = dropped_min = dropped_prop = on_bound = 0
    for s in range(n_scenes):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        a, pos_min[s], limit[s] = align(pos[lo:hi])
        if hi == lo:
            continue
        nx = axis_blocks(limit[s, 0], block_size, stride, count_form)
        ny = axis_blocks(limit[s, 1], block_size, stride, count_form)
        cells += nx * ny
        for i in range(nx):
            xl, xh, cxl, cxh = block_bounds(i, block_size, stride, padding)
            for j in range(ny):
                yl, yh, cyl, cyh = block_bounds(j, block_size, stride, padding)
                cond = (a[:, 0] >= xl) & (a[:, 0] <= xh) & (a[:, 1] >= yl) & (a[:, 1] <= yh)
                count = int(cond.sum())
                if count < min_points:
                    dropped_min += 1
                    continue
                b = a[cond]
                m = (b[:, 0] >= cxl) & (b[:, 0] <= cxh) & (b[:, 1] >= cyl) & (b[:, 1] <= cyh)
                if count == 0 or not float(int(m.sum())) / float(count) >= proportion:
                    dropped_prop += 1
                    continue
                local = np.nonzero(cond)[0].astype(np.int64)
                on_bound += int(((b[:, 0] == xl) | (b[:, 0] == xh) | (b[:, 1] == yl) | (b[:, 1] == yh)).sum())
                indices.append(local)
                rows.append(local + lo)
                mask.append(m.astype(np.int8))
                batch.append(np.full(count, len(scene), np.int64))
                scene.append(s)
                cell.append((i, j))
                out_ptr.append(out_ptr[-1] + count)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)          # noqa: E731
    return dict(ptr=np.asarray(out_ptr, np.int64), indices=cat(indices, np.int64), rows=cat(rows, np.int64), mask=cat(mask, np.int8),
                batch=cat(batch, np.int64), scene=np.asarray(scene, np.int64), cell=np.asarray(cell, np.int32).reshape(-1, 2),
                pos_min=pos_min, limit=limit, n_blocks=len(scene), n_rows=out_ptr[-1], cells=cells, dropped_min_points=dropped_min,
                dropped_proportion=dropped_prop, on_bound=on_bound)


def brute_sliding_blocks(p, *, block_size, stride, padding, min_points=200, proportion=0.02, count_form='ratio'):
    """One scene, the definition as a loop over all cells and all points: [(i, j, [point indices], [mask flags])] of the kept blocks.
    Float32 values are compared as the Python floats they convert to exactly."""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if len(p) == 0:
        return []
    mn = [min(np.float32(v) for v in p[:, k]) for k in range(3)]
    ax = [float(np.float32(v) - mn[0]) for v in p[:, 0]]              # (float32 - float32: one float32 rounding)
    ay = [float(np.float32(v) - mn[1]) for v in p[:, 1]]
    nx = axis_blocks(np.float32(max(ax)), block_size, stride, count_form)
    ny = axis_blocks(np.float32(max(ay)), block_size, stride, count_form)
    kept = []
    for i in range(nx):
        for j in range(ny):
            xbeg, ybeg = i * stride, j * stride
            xl, xh = float(np.float32(xbeg - padding)), float(np.float32(xbeg + block_size + padding))
            yl, yh = float(np.float32(ybeg - padding)), float(np.float32(ybeg + block_size + padding))
            cxl, cxh, cyl, cyh = float(np.float32(xbeg)), float(np.float32(xbeg + block_size)), float(np.float32(ybeg)), float(np.float32(ybeg + block_size))
            members, flags = [], []
            for q in range(len(ax)):
                if xl <= ax[q] <= xh and yl <= ay[q] <= yh:
                    members.append(q)
                    flags.append(1 if (cxl <= ax[q] <= cxh and cyl <= ay[q] <= cyh) else 0)
            if len(members) < min_points or len(members) == 0 or sum(flags) / len(members) < proportion:
                continue
            kept.append((i, j, members, flags))
    return kept


def np_features(pos, scene_ptr, split, form, extra=None):
    """(pos_block, x) of BlockSplit.features in float32 NumPy, block by block."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    F = 0 if extra is None else extra.shape[1]
    pos_block, x = np.zeros((split['n_rows'], 3), np.float32), np.zeros((split['n_rows'], 3 + F), np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        for b in range(split['n_blocks']):
            lo, hi, s = int(split['ptr'][b]), int(split['ptr'][b + 1]), int(split['scene'][b])
            r = split['rows'][lo:hi]
            a = (pos[r] - split['pos_min'][s]).astype(np.float32)
            e = np.zeros((hi - lo, 0), np.float32) if extra is None else np.asarray(extra, np.float32)[r]
            pos_block[lo:hi] = a
            if form == 'room':
                x[lo:hi] = np.concatenate([e, (a / split['limit'][s]).astype(np.float32)], 1)
            elif form == 'block':
                bmin, bmax = a.min(0), a.max(0)
                centre = ((bmin + bmax).astype(np.float32) / np.float32(2)).astype(np.float32)
                centre[2] = bmin[2]
                x[lo:hi] = np.concatenate([(a - centre).astype(np.float32), e], 1)
            else:
                raise ValueError(form)
    return pos_block, x


def max_multiplicity(block_size, stride, padding, **_):
    """The most blocks a point of a large scene lies in: (floor((block_size + 2 padding) / stride) + 1) ** 2."""
    return (int(math.floor((block_size + 2 * padding) / stride)) + 1) ** 2


def multiplicity(split, n_points):
    """How many kept blocks each point lies in."""
    return np.bincount(split['rows'], minlength=n_points)


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _shuffled(seed, p):
    return np.ascontiguousarray(p[S.permutation(seed, 'rows', len(p))]).astype(np.float32)


def carved_scene():
    """About 5000 points in 4.3 x 3.6 x 2.5 m with the far corner carved out: its corner block is all but empty."""
    p = S.make_cloud(3301, 5600, box=(4.3, 3.6, 2.5))
    return np.ascontiguousarray(p[~((p[:, 0] > 2.75) & (p[:, 1] > 2.75))])


def carved_small_scene():
    """The same carved at 3.2 x 2.7 m, for the S3DIS parameters."""
    p = S.make_cloud(3302, 5600, box=(3.2, 2.7, 2.5))
    return np.ascontiguousarray(p[~((p[:, 0] > 2.65) & (p[:, 1] > 2.15))])


def strip_scene():
    """3000 points in x < 1, 1500 in x in [2.55, 2.7] and 40 in the far corner, 4.3 x 3.6 m: at the ScanNet parameters the blocks of
    column 1 hold points only in their padding ring, and the blocks of column 3 hold the forty."""
    a = S.make_cloud(3303, 3000, box=(1.0, 3.6, 2.0))
    b = S.make_cloud(3304, 1500, box=(0.15, 3.6, 2.0)) + np.float32([2.55, 0, 0])
    c = S.make_cloud(3305, 40, box=(0.3, 0.3, 2.0)) + np.float32([4.0, 3.3, 0])
    return _shuffled(3306, np.concatenate([a, b, c]))


def lattice_scene():
    """Every multiple of 0.125 in 4 x 3 x 1 m, shuffled: with the DYADIC parameters many points sit exactly on a bound."""
    g = np.stack(np.meshgrid(np.arange(33), np.arange(25), np.arange(9), indexing='ij'), -1).reshape(-1, 3)
    return _shuffled(3307, (g * 0.125).astype(np.float32))


def tiny_scene():
    """300 points in 0.3 m: no block under 'ratio', one candidate under 'ceil_first' with the S3DIS geometry."""
    return S.make_cloud(3308, 300, box=(0.3, 0.3, 0.3))


def planar_scene():
    """A floor: every z equal, so limit.z is 0."""
    p = S.make_cloud(3309, 3000, box=(3.2, 2.7, 1.0))
    p[:, 2] = np.float32(0.75)
    return p


def zeros_scene():
    """A minimum that is a zero of both signs on every axis, +0.0 first on x, -0.0 first on y."""
    p = S.make_cloud(3311, 1500, box=(3.2, 2.7, 1.0))
    p[0], p[1], p[2] = (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, 0.0, 0.0)
    return p


def yard_scene():
    """9000 points in 13 x 11 x 3 m, for the 5 m blocks: 3 x 3 of them under 'ceil_first', where 'ratio' would lay 4 x 3."""
    return S.make_cloud(3310, 9000, box=(13.0, 11.0, 3.0))


SCENES = {'carved': carved_scene, 'carved_small': carved_small_scene, 'strip': strip_scene, 'lattice': lattice_scene, 'tiny': tiny_scene,
          'planar': planar_scene, 'yard': yard_scene, 'zeros': zeros_scene}

# the ragged batch: an empty scene, one point, one below and one above a wavefront, one past 1024, about 4100, the tiny and the strip scene
RAGGED_SIZES = [0, 1, 63, 65, 1025, 4100]


def ragged_scenes():
    """The scenes of the ragged batch, each in its own place, rows shuffled.  The 4100-point scene receives as many extra points in a
    spot that only block (0, 0) covers as it takes for the batch's row total at the ScanNet parameters to be one past a multiple of
    the sort's chunk."""
    scenes = []
    for k, n in enumerate(RAGGED_SIZES):
        box = (4.3, 3.6, 2.5) if n > 4000 else (2.0, 1.8, 1.0)
        scenes.append((S.make_cloud(3320 + k, n, box=box) + np.float32(2.5 * k)).astype(np.float32))
    scenes += [tiny_scene() - np.float32(1.0), strip_scene() + np.float32(7.0)]
    big = RAGGED_SIZES.index(4100)
    total = sum(np_sliding_blocks(p, **SCANNET)['n_rows'] for p in scenes)
    extra = (1 - total) % SORT_CHUNK
    spot = (S.make_cloud(3330, extra, box=(0.4, 0.4, 1.0)) + np.float32([0.3, 0.3, 0.5]) + np.float32(2.5 * big)).astype(np.float32)
    scenes[big] = _shuffled(3331, np.concatenate([scenes[big], spot]))
    return scenes


def ptr_of(scenes):
    return np.concatenate([[0], np.cumsum([len(p) for p in scenes])]).astype(np.int64)
