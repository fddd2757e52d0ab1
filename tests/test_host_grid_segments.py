"""The grid subsampling of ragged batches as far as it goes without a GPU: the new public header's prototypes, what ``grid.grid_subsample``
refuses before it reaches the library, the NumPy restatement (tests/grid_segments_restatement.py) against the reference's own compiled
core, and the conditions on the inputs of tests/test_gpu_grid_segments.py, so that test cannot hide behind its fixtures."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_counts import N_FUNCTIONS, N_RECORDS
import grid_segments_restatement as R
from crfconv_amd import _lib
from oracle import native as onative

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_public_grid_header_declares_the_entries():
    with open(os.path.join(ROOT, 'include', 'crfconv_amd.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS          # (the first header's counts are pinned: its tables stay its own)
    with open(os.path.join(ROOT, 'include', 'crfconv_grid.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert functions == _lib.GRID_SIGNATURES and records == {} and _lib.GRID_RECORDS == {}
    assert sorted(functions) == ['crfconv_grid_subsample_segments', 'crfconv_grid_subsample_segments_workspace']
    for other in (_lib.SIGNATURES, _lib.INTERNAL_SIGNATURES, _lib.BLOCKS_SIGNATURES, _lib.VOTES_SIGNATURES):
        assert not set(functions) & set(other)
    v, i, l, z, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
    assert functions['crfconv_grid_subsample_segments_workspace'] == (z, [l, l])
    assert functions['crfconv_grid_subsample_segments'] == (i, [v, l, v, l, v, i, v, i, f, l, v, z, v, v, v, v, v, v, v, v])
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in functions)
    assert lib.crfconv_grid_subsample_segments_workspace(0, 1) == 0 and lib.crfconv_grid_subsample_segments_workspace(5, 0) == 0
    assert lib.crfconv_grid_subsample_segments_workspace(5000, 3) >= 5000 * (8 + 8 + 4 + 4 + 4 + 4 + 4)


def test_a_c_caller_sees_the_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
    assert cc is not None, 'no C compiler on PATH'
    src = tmp_path / 'caller.c'
    src.write_text('#include "crfconv_grid.h"\n'
                   'size_t (*query)(int64_t, int64_t) = crfconv_grid_subsample_segments_workspace;\n'
                   'int (*entry)(const float*, int64_t, const int64_t*, int64_t, const float*, int, const int32_t*, int, float, int64_t, void*,\n'
                   '             size_t, float*, float*, int32_t*, int64_t*, int64_t*, int32_t*, int64_t*, crf_stream_t)\n'
                   '    = crfconv_grid_subsample_segments;\n')
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'caller.o')])


def test_grid_subsample_refuses_bad_arguments_before_the_library(monkeypatch):
    from crfconv_amd import grid

    def never(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', never)
    monkeypatch.setattr(_lib, 'load', never)
    pos = torch.zeros((10, 3), dtype=torch.float32)
    for size in (0.0, -1.0, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='size must be positive'):
            grid.grid_subsample(pos, size=size)
    for bad in (torch.zeros((10, 2)), torch.zeros(30), torch.zeros((10, 3), dtype=torch.float64), np.zeros((10, 3), np.float32)):
        with pytest.raises(ValueError, match=r'pos must be a float32 tensor \[N, 3\]'):
            grid.grid_subsample(bad, size=0.1)
    for x in (torch.zeros((9, 3)), torch.zeros(10), torch.zeros((10, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match='x must be a float32 tensor'):
            grid.grid_subsample(pos, size=0.1, x=x)
    for y in (torch.zeros(11, dtype=torch.int64), torch.zeros((9, 2), dtype=torch.int32), torch.zeros(10), torch.zeros((10, 1, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match='y must be an int32 or int64 tensor'):
            grid.grid_subsample(pos, size=0.1, y=y)
    for ptr in ([0, 4, 9], [0, 4, 11], [1, 10], [0, 6, 4, 10], torch.tensor([0, 12]), [0], []):
        with pytest.raises(ValueError, match='ptr must'):
            grid.grid_subsample(pos, ptr, size=0.1)
    with pytest.raises(ValueError, match='ptr must be int64'):
        grid.grid_subsample(pos, torch.tensor([0, 10], dtype=torch.int32), size=0.1)
    with pytest.raises(ValueError, match='on the device'):      # everything else in order: only the device is missing
        grid.grid_subsample(pos, [0, 4, 10], size=0.1, x=torch.zeros((10, 2)), y=torch.zeros(10, dtype=torch.int32))


def _by_key(pts_in, size, rows_pts):
    """order that sorts the reference's rows (hash-map order) by voxel key: rows are matched through their exact barycentres"""
    op, _, _, okeys = onative.oracle_grid_subsample(pts_in, None, None, size)
    lut = {tuple(p): k for p, k in zip(map(tuple, op), okeys)}
    assert len(lut) == len(op)
    return np.argsort(np.array([lut[tuple(p)] for p in map(tuple, rows_pts)], dtype=np.uint64), kind='stable')


def test_restatement_agrees_with_the_compiled_reference_core():
    if not onative.have_ref():
        pytest.skip('oracle/_ref not built (needs the reference sources)')
    pos, ptr, x, y, size = R.tie_free_batch()
    assert len(ptr) == 4 and (np.diff(ptr) > 0).all()
    want = R.np_grid_subsample(pos, ptr, size, x, y)
    # no voxel can tie, so every label row takes part in the comparison
    n0 = np.bincount(want['inverse'], weights=(y == 0), minlength=len(want['pos']))
    n1 = np.bincount(want['inverse'], weights=(y == 1), minlength=len(want['pos']))
    assert set(np.unique(y)) == {0, 1} and (n0 != n1).all() and (n0 + n1 == want['counts']).all()
    assert ((n0 > 0) & (n1 > 0)).sum() > 50                  # (and mixed voxels exist: the mode is a decision)
    assert (want['counts'] % 2 == 0).sum() > 50
    rp, rx, ry = [], [], []
    for s in range(3):
        sel = slice(ptr[s], ptr[s + 1])
        p, f, c = onative.ref_grid_subsample(pos[sel], x[sel], y[sel], size)
        order = _by_key(pos[sel], size, p)
        rp.append(p[order]); rx.append(f[order]); ry.append(c[order])
    assert np.array_equal(want['ptr'], np.concatenate([[0], np.cumsum([len(p) for p in rp])]))
    assert np.array_equal(want['pos'].view(np.uint32), np.concatenate(rp).view(np.uint32))
    assert np.array_equal(want['x'].view(np.uint32), np.concatenate(rx).view(np.uint32))
    assert np.array_equal(want['y'], np.concatenate(ry))


def test_restatement_of_a_batch_is_its_clouds_shifted():
    pos, ptr, x, y = R.main_batch()
    whole = R.np_grid_subsample(pos, ptr, R.SIZE, x, y)
    assert whole['ptr'][0] == 0 and whole['ptr'][-1] == len(whole['pos']) == len(whole['counts']) and whole['counts'].sum() == len(pos)
    assert whole['y'].shape == (len(whole['pos']), 2) and whole['inverse'].shape == (len(pos),)
    for s in range(len(ptr) - 1):
        sel, osel = slice(ptr[s], ptr[s + 1]), slice(whole['ptr'][s], whole['ptr'][s + 1])
        one = R.np_grid_subsample(pos[sel], None, R.SIZE, x[sel], y[sel])
        assert np.array_equal(whole['pos'][osel], one['pos']) and np.array_equal(whole['x'][osel], one['x'])
        assert np.array_equal(whole['y'][osel], one['y']) and np.array_equal(whole['counts'][osel], one['counts'])
        assert np.array_equal(whole['inverse'][sel], one['inverse'] + whole['ptr'][s])


# ------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
def test_main_batch_has_the_sizes_borders_and_ties():
    pos, ptr, x, y = R.main_batch()
    assert np.diff(ptr).tolist() == [1, 700, 0, 4097, 257] and x.shape == (len(pos), 3) and y.shape == (len(pos), 2)
    assert (ptr[1:-1] % 64 != 0).all() and 0 < ptr[3] < 4096 < ptr[4]       # borders inside a wavefront and inside a 4096-row chunk
    assert pos[ptr[1]:ptr[2]].max() < 0 and pos[ptr[3]:ptr[4]].min() > 2     # one cloud in negative coordinates
    lo = np.array([pos[ptr[s]:ptr[s + 1]].min(0) for s in (0, 1, 3, 4)])
    assert len({tuple(np.floor(v / 1.5)) for v in lo}) == 4                  # every cloud shifted differently
    want = R.np_grid_subsample(pos, ptr, R.SIZE, x, y)
    assert want['ptr'][2] == want['ptr'][3] and want['ptr'][1] == 1          # the empty cloud, the one-point cloud
    assert want['counts'].min() == 1 and 12 <= want['counts'].max() <= 64 and (want['counts'] > 1).sum() > 300
    # ties between the most frequent labels occur, among them ties that the smallest label wins against the first-seen one
    ties = first_loses = 0
    for v in np.flatnonzero(want['counts'] > 1)[:2000]:
        rows = np.flatnonzero(want['inverse'] == v)
        for l in range(2):
            c = np.bincount(y[rows, l], minlength=3)
            if (c == c.max()).sum() > 1:
                ties += 1
                first = next(int(t) for t in y[rows, l] if c[t] == c.max())
                first_loses += int(first != int(np.argmax(c)))
                assert want['y'][v, l] == int(np.argmax(c))
    assert ties > 100 and first_loses > 20


def test_heavy_cloud_has_one_voxel_wider_than_a_workgroup():
    pos = R.heavy_cloud()
    want = R.np_grid_subsample(pos, None, 1.0)
    assert len(pos) == 5000 and sorted(want['counts'].tolist()) == [1] * 2000 + [3000]
    assert want['counts'][0] == 3000                         # (the dense voxel is the cloud's first)


def test_the_extremes_are_extreme():
    pos, ptr, x, y = R.main_batch()
    one = R.np_grid_subsample(pos, ptr, 64.0)
    assert one['ptr'].tolist() == [0, 1, 2, 2, 3, 4] and one['counts'].tolist() == [1, 700, 4097, 257]
    own = R.np_grid_subsample(pos, ptr, 1e-4)
    assert np.array_equal(own['ptr'], ptr) and (own['counts'] == 1).all()
    for s in range(5):
        assert sorted(own['inverse'][ptr[s]:ptr[s + 1]].tolist()) == list(range(ptr[s], ptr[s + 1]))
