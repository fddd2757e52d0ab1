"""-m gpu: ``grid.grid_subsample`` (csrc/grid_subsample.hip) on ragged batches against the NumPy restatement around the CPU oracle
(tests/grid_segments_restatement.py), bit for bit in every output: pos, x, y, ptr, inverse, counts.  The inputs and the conditions on
them are checked without a GPU in tests/test_host_grid_segments.py."""
import numpy as np
import pytest
import torch

import grid_segments_restatement as R
from crfconv_amd import grid

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(pos, ptr, size, x=None, y=None):
    return grid.grid_subsample(dev(pos), None if ptr is None else dev(ptr), size=size, x=dev(x), y=dev(y))


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, N, x=None, y=None):
    """every output against the restatement: shapes, dtypes, devices and bits"""
    M = len(want['pos'])
    assert all(t is None or t.device == torch.device(DEV) for t in got)
    assert got.pos.dtype == torch.float32 and tuple(got.pos.shape) == (M, 3) and np.array_equal(bits(got.pos), bits(want['pos']))
    assert got.ptr.dtype == torch.int64 and np.array_equal(got.ptr.cpu().numpy(), want['ptr'])
    assert got.inverse.dtype == torch.int64 and tuple(got.inverse.shape) == (N,) and np.array_equal(got.inverse.cpu().numpy(), want['inverse'])
    assert got.counts.dtype == torch.int32 and tuple(got.counts.shape) == (M,) and np.array_equal(got.counts.cpu().numpy(), want['counts'])
    if x is None:
        assert got.x is None
    else:
        assert got.x.dtype == torch.float32 and tuple(got.x.shape) == (M, x.shape[1]) and np.array_equal(bits(got.x), bits(want['x']))
    if y is None:
        assert got.y is None
    else:
        assert got.y.dtype == dev(y).dtype and got.y.dim() == y.ndim
        assert np.array_equal(got.y.cpu().numpy().reshape(M, -1), want['y'])


@pytest.fixture(scope='module')
def main():
    pos, ptr, x, y = R.main_batch()
    return dict(pos=pos, ptr=ptr, x=x, y=y)


@pytest.mark.parametrize('form', ['y int64 [N, 2]', 'y int32 [N]', 'x alone', 'neither'])
def test_main_ragged_batch(main, form):
    pos, ptr = main['pos'], main['ptr']
    x = None if form == 'neither' else main['x']
    y = {'y int64 [N, 2]': main['y'], 'y int32 [N]': main['y'][:, 1].astype(np.int32)}.get(form)
    want = R.np_grid_subsample(pos, ptr, R.SIZE, x, y)
    assert want['ptr'].tolist()[1:4] == [1, want['ptr'][2], want['ptr'][2]]          # the one-point cloud, the empty cloud
    same(run(pos, ptr, R.SIZE, x, y), want, len(pos), x, y)


def test_ptr_as_list_and_host_tensor(main):
    pos, ptr, x = main['pos'], main['ptr'], main['x']
    want = R.np_grid_subsample(pos, ptr, R.SIZE, x)
    for form in (ptr.tolist(), torch.from_numpy(ptr)):
        same(grid.grid_subsample(dev(pos), form, size=R.SIZE, x=dev(x)), want, len(pos), x)


def test_single_cloud_equals_the_host_entry(main):
    from crfconv_amd.utils import cpp_subsampling
    sel = slice(main['ptr'][3], main['ptr'][4])
    pos, x, y = main['pos'][sel], main['x'][sel], main['y'][sel].astype(np.int32)
    assert len(pos) == 4097
    got = run(pos, None, R.SIZE, x, y)
    hp, hx, hy = cpp_subsampling.compute(pos, features=x, classes=y, sampleDl=R.SIZE)
    assert np.array_equal(bits(got.pos), bits(hp)) and np.array_equal(bits(got.x), bits(hx)) and np.array_equal(got.y.cpu().numpy(), hy)
    same(got, R.np_grid_subsample(pos, None, R.SIZE, x, y), len(pos), x, y)


def _rekey_rows(pts_in, dl, rows):
    from oracle import native as onative
    op, _, _, okeys = onative.oracle_grid_subsample(pts_in, None, None, dl)
    lut = {tuple(p): k for p, k in zip(map(tuple, op), okeys)}
    return np.array([lut[tuple(p)] for p in map(tuple, rows)], dtype=np.uint64)


def test_fixture_cloud_second_in_a_batch(golden, main):
    g = golden('g7_grid.npz')
    dl = float(g['all/dl'])
    first = main['pos'][main['ptr'][1]:main['ptr'][2]]
    pos, ptr = np.concatenate([first, g['pts']]), np.array([0, len(first), len(first) + len(g['pts'])], np.int64)
    x = np.concatenate([main['x'][:len(first)], g['feats']])
    y = np.concatenate([np.zeros(len(first), np.int32), g['lab1'].reshape(-1).astype(np.int32)])
    got = run(pos, ptr, dl, x, y)
    same(got, R.np_grid_subsample(pos, ptr, dl, x, y), len(pos), x, y)
    lo = int(got.ptr[1])
    order = np.argsort(_rekey_rows(g['pts'], dl, g['all/pts']), kind='stable')              # the reference's rows, re-keyed
    assert np.array_equal(bits(got.pos[lo:]), bits(g['all/pts'][order]))
    assert np.array_equal(bits(got.x[lo:]), bits(g['all/feats'][order]))


def test_heavy_voxel():
    pos = R.heavy_cloud()
    x = R.S.uniform(82, 'x', (len(pos), 3), 0.0, 255.0)
    y = R.S.integers(82, 'y', (len(pos), 1), 0, 5).astype(np.int64)
    want = R.np_grid_subsample(pos, None, 1.0, x, y)
    assert want['counts'].max() == 3000
    same(run(pos, None, 1.0, x, y), want, len(pos), x, y)


@pytest.mark.parametrize('size,what', [(64.0, 'one voxel per cloud'), (1e-4, 'one voxel per point')])
def test_extremes(main, size, what):
    pos, ptr, x, y = main['pos'], main['ptr'], main['x'], main['y']
    want = R.np_grid_subsample(pos, ptr, size, x, y)
    got = run(pos, ptr, size, x, y)
    same(got, want, len(pos), x, y)
    if what == 'one voxel per cloud':
        assert got.pos.shape[0] == 4 and got.ptr.tolist() == [0, 1, 2, 2, 3, 4]             # M = S minus the empty cloud
    else:
        assert got.pos.shape[0] == len(pos) and np.array_equal(got.ptr.cpu().numpy(), ptr)
        inv = got.inverse.cpu().numpy()
        for s in range(len(ptr) - 1):                                                        # a permutation per cloud
            assert np.array_equal(np.sort(inv[ptr[s]:ptr[s + 1]]), np.arange(ptr[s], ptr[s + 1]))


def test_two_runs_give_the_same_bits(main):
    a = run(main['pos'], main['ptr'], R.SIZE, main['x'], main['y'])
    b = run(main['pos'], main['ptr'], R.SIZE, main['x'], main['y'])
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v))


def test_empty_batches_launch_nothing():
    pos = torch.zeros((0, 3), dtype=torch.float32, device=DEV)
    got = grid.grid_subsample(pos, [0, 0, 0], size=0.1, x=torch.zeros((0, 2), device=DEV), y=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert got.ptr.tolist() == [0, 0, 0] and tuple(got.pos.shape) == (0, 3) and tuple(got.x.shape) == (0, 2)
    assert tuple(got.y.shape) == (0,) and got.y.dtype == torch.int64 and got.inverse.numel() == 0 and got.counts.numel() == 0
    assert grid.grid_subsample(pos, size=0.1).ptr.tolist() == [0, 0]


def test_bad_ptr_and_key_overflow_raise(main):
    pos = dev(main['pos'])
    N = pos.shape[0]
    for bad in ([0, 700, 300, N], [0, 5, N - 1], [1, 5, N], [0, -1, N]):
        with pytest.raises(ValueError, match='ptr must start at 0'):
            grid.grid_subsample(pos, torch.tensor(bad, dtype=torch.int64, device=DEV), size=R.SIZE)
    # two clouds of two points 1e6 apart on every axis: 1e9 cells along each, 1e27 in a cloud
    far = np.array([[0, 0, 0], [1e6, 1e6, 1e6], [5, 5, 5], [5 + 1e6, 5 + 1e6, 5 + 1e6]], np.float32)
    with pytest.raises(ValueError, match='64-bit key'):
        grid.grid_subsample(dev(far), [0, 2, 4], size=1e-3)
    # the same clouds on a grid that fits are fine, and one cloud alone keeps the reference's wrap-around
    same(run(far, np.array([0, 2, 4], np.int64), 1.0), R.np_grid_subsample(far, [0, 2, 4], 1.0), 4)
    same(run(far[:2], None, 1e-3), R.np_grid_subsample(far[:2], None, 1e-3), 2)
