"""The grid subsampling of a ragged batch, restated with NumPy around the CPU oracle (oracle/grid_oracle.c): every cloud is subsampled on its
own -- ``oracle.native.oracle_grid_subsample`` and ``grid_keys`` -- and the results are put one behind the other.  What
``crfconv_amd.grid.grid_subsample`` must return bit for bit, and the clouds of tests/test_gpu_grid_segments.py with the conditions on them
(tests/test_host_grid_segments.py checks those without a GPU)."""
import numpy as np

import _seeded as S
from oracle import native as onative

SIZE = 0.06
MAIN_SIZES = (1, 700, 0, 4097, 257)
# every cloud somewhere else, the second in negative coordinates, the fourth far enough out that float32 spacing shows
MAIN_SHIFTS = ((0.0, 0.0, 0.0), (-7.25, -3.5, -2.125), (0.0, 0.0, 0.0), (31.5, 12.75, 2.0), (3.0, -40.0, 0.5))


def ptr_of(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def np_grid_subsample(pos, ptr=None, size=SIZE, x=None, y=None):
    """dict(pos [M, 3], x [M, F] | None, y [M, L] int32 | None, ptr [S + 1], inverse [N], counts [M]): cloud by cloud, rows inside a cloud
    in ascending voxel key; inverse = ptr_out[s] + searchsorted(okeys, keys)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    N = len(pos)
    ptr = np.array([0, N], np.int64) if ptr is None else np.asarray(ptr, np.int64)
    F = 0 if x is None else x.shape[1]
    y2 = None if y is None else (np.asarray(y) if np.ndim(y) == 2 else np.asarray(y)[:, None]).astype(np.int32)
    L = 0 if y2 is None else y2.shape[1]
    out = {'pos': [np.zeros((0, 3), np.float32)], 'x': [np.zeros((0, F), np.float32)], 'y': [np.zeros((0, L), np.int32)],
           'inverse': [np.zeros(0, np.int64)], 'counts': [np.zeros(0, np.int32)]}
    out_ptr = [0]
    for s in range(len(ptr) - 1):
        sel = slice(ptr[s], ptr[s + 1])
        if ptr[s + 1] == ptr[s]:
            out_ptr.append(out_ptr[-1])
            continue
        p = pos[sel]
        op, of, oc, okeys = onative.oracle_grid_subsample(p, None if x is None else x[sel], None if y2 is None else y2[sel], size)
        keys = onative.grid_keys(p, size)
        assert (okeys[1:] > okeys[:-1]).all()
        local = np.searchsorted(okeys, keys)
        assert np.array_equal(okeys[local], keys)
        out['pos'].append(op)
        if x is not None:
            out['x'].append(of)
        if y2 is not None:
            out['y'].append(oc)
        out['inverse'].append(out_ptr[-1] + local.astype(np.int64))
        out['counts'].append(np.bincount(local, minlength=len(okeys)).astype(np.int32))
        out_ptr.append(out_ptr[-1] + len(okeys))
    res = {k: np.concatenate(v) for k, v in out.items()}
    if x is None:
        res['x'] = None
    if y is None:
        res['y'] = None
    res['ptr'] = np.asarray(out_ptr, np.int64)
    return res


def cloud(seed, n, shift=(0.0, 0.0, 0.0), box=(1.5, 1.5, 1.5)):
    """n points in a box, moved by `shift` (float32 addition): half of them uniform, half in blobs of about 150 points and 4 cm spread,
    so that voxels of a few centimetres hold from one point to a few dozen."""
    p = S.make_cloud(seed, n, box=box)
    r = S._rng(seed, 'blobs')
    half = n // 2
    if half:
        centres = (0.2 + 0.6 * r.random((max(1, half // 150), 3))) * np.asarray(box)
        p[:half] = centres[r.integers(0, len(centres), half)] + r.normal(0.0, 0.04, (half, 3))
        p = p[r.permutation(n)]
    return (p.astype(np.float32) + np.asarray(shift, np.float32)).astype(np.float32)


def main_batch():
    """(pos, ptr, x [N, 3], y [N, 2] int64 of three classes): five clouds of 1, 700, 0, 4097 and 257 points, each moved elsewhere."""
    parts = [cloud(70 + i, n, sh) for i, (n, sh) in enumerate(zip(MAIN_SIZES, MAIN_SHIFTS))]
    pos, ptr = np.concatenate(parts), ptr_of(parts)
    x = S.uniform(71, 'x', (len(pos), 3), 0.0, 255.0)
    y = S.integers(71, 'y', (len(pos), 2), 0, 3).astype(np.int64)
    return pos, ptr, x, y


def heavy_cloud():
    """3000 points inside ONE voxel of edge 1 and 2000 points alone in voxels of their own (a lattice of spacing 2), shuffled."""
    dense = 0.25 + 0.5 * S.make_cloud(81, 3000)
    k = np.arange(2000)
    lattice = np.stack([2.5 + 2.0 * (k % 20), 2.5 + 2.0 * ((k // 20) % 10), 2.5 + 2.0 * (k // 200)], 1)
    pos = np.concatenate([dense, lattice]).astype(np.float32)
    return pos[S.permutation(81, 'order', len(pos))]


def tie_free_batch():
    """(pos, ptr, x, y [N] int32, size) of three clouds whose labels cannot tie in any voxel: two classes, and a voxel with an even number
    of points has one label only."""
    parts = [cloud(90, 600, (0.0, 0.0, 0.0)), cloud(91, 1500, (-4.0, 2.0, -1.0)), cloud(92, 333, (9.0, 9.0, 9.0))]
    pos, ptr, size = np.concatenate(parts), ptr_of(parts), 0.2
    y = S.integers(93, 'y', (len(pos),), 0, 2).astype(np.int32)
    for s, p in enumerate(parts):
        keys = onative.grid_keys(p, size)
        _, local, counts = np.unique(keys, return_inverse=True, return_counts=True)
        even = (counts % 2 == 0)[local]
        first = np.zeros(len(counts), np.int32)
        first[local[::-1]] = y[ptr[s]:ptr[s + 1]][::-1]          # the label of the voxel's first point
        y[ptr[s]:ptr[s + 1]][even] = first[local][even]
    x = S.uniform(93, 'x', (len(pos), 4), -1.0, 1.0)
    return pos, ptr, x, y, size
