"""CPU checks of the ragged-batch transforms (crfconv_amd.transforms.SegmentCompose, Center, NormalizeScale, FixedPoints): the
validation of the chain, the laws of the picks' host twin, the float64 restatement the GPU tests compare against -- itself compared
with a plain float64 torch composition --, and the header / ABI record of the new entry points.  No GPU and no library needed."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segment_transforms_restatement as R
from crfconv_amd import _lib
from crfconv_amd import transforms as T
from crfconv_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 0, 63, 64, 65, 1023, 1024, 1025, 4097]


def part_chain(generator=None):
    """The ShapeNet-Part preparation: fixed size, unit ball, augmentation, x = [pos, norm]."""
    return T.SegmentCompose([
        T.FixedPoints(2048, replace=False, allow_duplicates=True),
        T.NormalizeScale(),
        T.RandomRotate(degrees=180, axis=2),
        T.RandomScaleAnisotropic(scales=[0.8, 1.2]),
        T.RandomSymmetry(axis=[True, False, False]),
        T.RandomNoise(sigma=0.001),
        T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'norm']),
    ], generator=generator)


def test_chain_validation_and_messages():
    c = part_chain(torch.Generator().manual_seed(0))
    assert c.fixed.num == 2048 and c.fixed.mode == 2 and c.normalize is not None and c.add_norm and not c.add_rgb
    assert repr(c).startswith('SegmentCompose(FixedPoints(2048, replace=False, allow_duplicates=True), NormalizeScale(), RandomRotate(')
    assert T.FixedPoints(8).mode == 0 and T.FixedPoints(8, replace=False).mode == 1
    assert T.FixedPoints(8, replace=True, allow_duplicates=True).mode == 0             # replace wins, as in PyG
    T.SegmentCompose([T.Center()])
    T.SegmentCompose([T.Center(), T.NormalizeScale(), T.RandomNoise(0.01)])
    T.SegmentCompose([T.FixedPoints(16)])
    T.SegmentCompose([T.DropFeature(0.2), T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[False, True])])
    with pytest.raises(NotImplementedError, match='SegmentCompose: Center.. out of order; supported is a subsequence of FixedPoints -> '
                                                  'Center -> NormalizeScale -> RandomRotate'):
        T.SegmentCompose([T.RandomRotate(180, axis=2), T.Center()])
    with pytest.raises(NotImplementedError, match='FixedPoints'):
        T.SegmentCompose([T.NormalizeScale(), T.FixedPoints(4)])
    with pytest.raises(NotImplementedError, match='out of order'):
        T.SegmentCompose([T.Center(), T.Center()])

    class SamplePoints:
        pass
    with pytest.raises(NotImplementedError, match=r'SamplePoints.* is not supported \(supported: FixedPoints, Center, NormalizeScale, '):
        T.SegmentCompose([T.Center(), SamplePoints()])
    with pytest.raises(NotImplementedError, match='only the rgb feature can be dropped'):
        T.SegmentCompose([T.DropFeature(0.2, feature_name='norm')])
    with pytest.raises(NotImplementedError, match=r"x must be \[pos\], \[pos, rgb\] or \[pos, norm\]"):
        T.SegmentCompose([T.AddFeatsByKeys([True, True, True], ['pos', 'rgb', 'norm'])])
    with pytest.raises(NotImplementedError, match="feature 'intensity'"):
        T.SegmentCompose([T.AddFeatsByKeys([True, True], ['pos', 'intensity'])])
    with pytest.raises(NotImplementedError, match='pos cannot be deleted'):
        T.SegmentCompose([T.AddFeatsByKeys([True, True], ['pos', 'norm'], delete_feats=[True, False])])
    with pytest.raises(ValueError):
        T.FixedPoints(0)


def test_compose_still_refuses_norm():
    with pytest.raises(NotImplementedError, match="'norm'"):
        T.Compose([T.AddFeatsByKeys([True, True], ['pos', 'norm'])])
    with pytest.raises(NotImplementedError, match='Center'):
        T.Compose([T.Center()])
    with pytest.raises(NotImplementedError, match='norm'):
        T.Compose([T.RandomRotate(180, axis=2)])(Data(pos=torch.zeros(4, 3), norm=torch.zeros(4, 3)))


def test_seeding_state_and_draws_without_the_library():
    g = torch.Generator().manual_seed(11)
    a, b = part_chain(g), part_chain(g)
    assert a.seed != b.seed and part_chain(torch.Generator().manual_seed(11)).seed == a.seed
    assert a.state_dict() == {'seed': a.seed, 'counter': 0}
    b.load_state_dict({'seed': 42, 'counter': 9})
    assert b.state_dict() == {'seed': 42, 'counter': 9}
    # cloud b of a ragged batch draws what Compose predicts for row b of a dense one
    dense = T.Compose([t for t in a.transforms if type(t) in (T.RandomRotate, T.RandomScaleAnisotropic, T.RandomSymmetry, T.RandomNoise)],
                      generator=torch.Generator().manual_seed(1))
    want, got = dense.draws(77, 3, 12), a.draws(77, 3, 12)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])
    code = ('import crfconv_amd.transforms as T, crfconv_amd._lib as L\n'
            'c = T.SegmentCompose([T.FixedPoints(8, replace=False), T.NormalizeScale(), T.RandomRotate(180, axis=2)])\n'
            'c.draws(1, 2, 3); c.state_dict(); c.fixed.draws(1, 2, [5, 0, 9]); c._spec()\n'
            'assert L._lib is None\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


@pytest.mark.parametrize('num', [1, 64, 2048])
@pytest.mark.parametrize('mode', ['replace', 'subset', 'duplicates'])
def test_fixed_points_draw_laws(mode, num):
    f = T.FixedPoints(num, replace=mode == 'replace', allow_duplicates=mode == 'duplicates')
    d = f.draws(1234, 5, SIZES)
    again = f.draws(1234, 5, SIZES)
    np.testing.assert_array_equal(d['index'], again['index'])
    assert d['index'].dtype == np.int64 and d['out_ptr'].dtype == np.int64 and len(d['out_ptr']) == len(SIZES) + 1
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    differs = False
    other = f.draws(1234, 6, SIZES)
    for b, n in enumerate(SIZES):
        pick = d['index'][d['out_ptr'][b]:d['out_ptr'][b + 1]]
        if n == 0:                                                    # nothing to pick: -1, the gather clamps
            assert len(pick) == (0 if mode == 'subset' else num) and np.all(pick == -1)
            continue
        assert len(pick) == (min(num, n) if mode == 'subset' else num)                 # num picks per cloud (PyG: randperm[:num])
        assert np.all((pick >= starts[b]) & (pick < starts[b] + n))                    # every pick lies inside its cloud
        times = np.bincount(pick - starts[b], minlength=n)
        if mode == 'subset':
            assert times.max() == 1                                                    # no duplicates
            assert np.all(np.diff(pick) > 0)                                           # ascending rows
        if mode == 'duplicates':
            assert set(np.unique(times)) <= {num // n, num // n + 1}
            whole = (num // n) * n
            np.testing.assert_array_equal(pick[:whole], starts[b] + np.arange(whole) % n)      # whole copies in row order
            assert np.all(np.diff(pick[whole:]) > 0)
        differs |= not np.array_equal(pick, other['index'][other['out_ptr'][b]:other['out_ptr'][b + 1]])
    assert differs                                                    # the next counter draws afresh
    # a cloud's picks depend on its position and size only, not on the other clouds
    alone = f.draws(1234, 5, SIZES[:8])
    np.testing.assert_array_equal(alone['index'], d['index'][:alone['out_ptr'][-1]])


def test_fixed_points_replace_is_uniform():
    n, num = 37, 37 * 4000
    pick = T.FixedPoints(num).draws(99, 0, [n])['index']
    times = np.bincount(pick, minlength=n)
    chi2 = float(((times - num / n) ** 2 / (num / n)).sum())
    assert chi2 < 36 + 5 * np.sqrt(2 * 36), chi2                      # chi-square with 36 degrees of freedom, 5 sigma


def test_restatement_against_a_plain_torch_composition():
    """The yardstick itself: restate() against pos - pos.mean(0), p * k, p @ M, .. written with float64 torch operators."""
    sizes = [1, 3, 0, 5, 64, 130]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N, S = int(ptr[-1]), len(sizes)
    rng = np.random.default_rng(5)
    pos = (rng.uniform(-1, 1, (N, 3)) * [3, 2, 1] + [300, -200, 50]).astype(np.float32)
    nrm = rng.standard_normal((N, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[7] = 0
    rgb = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    noise = rng.uniform(-0.1, 0.1, (N, 3)).astype(np.float32)
    params = np.zeros((S, 8), np.float32)
    th = rng.uniform(-np.pi, np.pi, S)
    params[:, 0], params[:, 1], params[:, 2:5] = np.cos(th), np.sin(th), rng.uniform(0.8, 1.2, (S, 3))
    params[:, 5], params[:, 6] = rng.integers(0, 8, S), np.arange(S) % 2
    stats = np.zeros((S, 4), np.float32)
    for axis in (0, 1, 2):
        want_p, want_n, want_c = [], [], []
        for b in range(S):
            p = torch.from_numpy(pos[ptr[b]:ptr[b + 1]]).double()
            n = torch.from_numpy(nrm[ptr[b]:ptr[b + 1]]).double()
            c = torch.from_numpy(rgb[ptr[b]:ptr[b + 1]]).double()
            if len(p):
                mean = p.mean(0)
                stats[b, :3] = mean.numpy()
                p = p - torch.from_numpy(stats[b, :3]).double()                  # (the mean as applied: rounded to float32)
                top = float(p.abs().max())
                stats[b, 3] = np.float32(1 / top) * np.float32(0.999999) if top > 0 else 0
                p = p * float(stats[b, 3])
                co, si = float(params[b, 0]), float(params[b, 1])
                M = {0: [[1, 0, 0], [0, co, si], [0, -si, co]], 1: [[co, 0, -si], [0, 1, 0], [si, 0, co]],
                     2: [[co, si, 0], [-si, co, 0], [0, 0, 1]]}[axis]            # torch_geometric RandomRotate's matrices
                M = torch.tensor(M, dtype=torch.float64)
                s = torch.from_numpy(params[b, 2:5]).double()
                p = (p @ M) * s
                n = (n @ M) / s
                n = torch.where(n.norm(dim=1, keepdim=True) > 0, n / n.norm(dim=1, keepdim=True), n)
                for i in range(3):
                    if (int(params[b, 5]) >> i) & 1:
                        p[:, i] = p[:, i].max() - p[:, i]
                        n[:, i] = -n[:, i]
                p = p + torch.from_numpy(noise[ptr[b]:ptr[b + 1]]).double().clamp(-0.05, 0.05)
                if params[b, 6] == 0:
                    c = c * 0
            want_p.append(p), want_n.append(n), want_c.append(c)
        want_p, want_n, want_c = torch.cat(want_p).numpy(), torch.cat(want_n).numpy(), torch.cat(want_c).numpy()
        got = R.restate(pos, ptr, params, stats, norm=nrm, rgb=rgb, noise=noise, center=True, normalize=True, axis=axis, scale=True,
                        flip_axes=7, clip=0.05, drop=True, x_layout='pos_rgb')
        np.testing.assert_allclose(got['pos'], want_p, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got['norm'], want_n, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got['x'], np.concatenate([want_p, want_c], 1), rtol=0, atol=1e-13)
        assert np.all(got['norm'][7] == 0)                                       # a zero normal stays zero
        assert got['R'][2] == 0 and np.all(got['R'][[0, 1, 3, 4, 5]] > 0) and got['R'].max() < 4        # computed values only: the centred extent (3), not the input's hundreds
        np.testing.assert_allclose(np.linalg.norm(np.delete(got['norm'], 7, 0), axis=1), 1, atol=1e-12)
    # the steps a chain lacks are the identity, and x = [pos, norm] / [pos]
    ident = R.restate(pos, ptr, params, stats, norm=nrm, x_layout='pos_norm')
    np.testing.assert_array_equal(ident['x'], np.concatenate([pos, nrm], 1).astype(np.float64))
    only = R.restate(pos, ptr, params, stats, center=True, x_layout='pos')
    for b in range(S):
        if sizes[b]:
            np.testing.assert_allclose(only['pos'][ptr[b]:ptr[b + 1]], pos[ptr[b]:ptr[b + 1]].astype(np.float64) - stats[b, :3], atol=0)
    # the picks' effect on the row attributes
    idx = T.FixedPoints(8).draws(3, 0, [s for s in sizes if s])['index']
    gp, gn, none = R.gather(idx, pos, nrm, None)
    assert none is None and np.array_equal(gp, pos[idx]) and np.array_equal(gn, nrm[idx])


def test_header_and_abi_of_the_new_record():
    # the unit's declarations stand in include/crfconv_amd.h itself, the one header of the ABI, and in _lib's one pair of tables
    assert _lib.RECORDS['crf_augment_segments_spec'] is _lib.AugmentSegmentsSpec
    assert {'crfconv_augment_segments', 'crfconv_fixed_points'} <= set(_lib.SIGNATURES)
    assert glob.glob(os.path.join(os.path.dirname(_lib.HEADER_PATH), 'crfconv_amd_*.h')) == []
    spec = _lib.AugmentSegmentsSpec
    names = [n for n, _ in spec._fields_]
    assert names == ['center', 'normalize', 'rotate_axis', 'deg_lo', 'deg_hi', 'scale', 'scale_lo', 'scale_span', 'flip_axes', 'noise',
                     'sigma', 'clip', 'drop', 'drop_p', 'x_norm']
    floats = {'deg_lo', 'deg_hi', 'scale_lo', 'scale_span', 'sigma', 'clip', 'drop_p'}
    assert all(t is (ctypes.c_float if n in floats else ctypes.c_int32) for n, t in spec._fields_)
    assert ctypes.sizeof(spec) == 60                                  # flat, fifteen 4-byte fields, no padding
    # the dense record is a suffix-free subset: the shared device functions read the same names in both
    assert [n for n, _ in _lib.AugmentSpec._fields_] == names[2:-1]
    res, args = _lib.SIGNATURES['crfconv_augment_segments']
    assert res is ctypes.c_int and len(args) == 15
    assert args[:3] == [ctypes.c_void_p] * 3 and args[3] is ctypes.c_int64 and args[4] is ctypes.c_int and args[6] is ctypes.c_int64
    assert args[8] is ctypes.c_uint64 and args[-1] is ctypes.c_void_p
    res, args = _lib.SIGNATURES['crfconv_fixed_points']
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # the kernel's view of a chain
    s = part_chain(torch.Generator().manual_seed(0))._spec()
    assert (s.center, s.normalize, s.rotate_axis, s.scale, s.flip_axes, s.noise, s.drop, s.x_norm) == (1, 1, 2, 1, 1, 1, 0, 1)
    s = T.SegmentCompose([T.Center()])._spec()
    assert (s.center, s.normalize, s.rotate_axis, s.scale, s.flip_axes, s.noise, s.drop, s.x_norm) == (1, 0, -1, 0, 0, 0, 0, 0)
