"""No GPU: the S3DIS form of the crop sampler on the host -- the numpy restatement (s3dis_restatement.py) against the fixture the
reference's own S3DISRoom._get_random produced (g12_s3dis_sampler.npz), the numpy twin of the padding draws, and the argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from crfconv_amd import _lib
from crfconv_amd.sampling import PossibilitySampler, VoteAccumulator
from s3dis_restatement import S3DISTwin, vote_repeated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DRAWS = 8


def twin_of(g):
    return S3DISTwin([g['cloud%d' % c] for c in range(3)], [g['rgb%d' % c] for c in range(3)], [g['labels%d' % c] for c in range(3)],
                     [g['poss%d' % c] for c in range(3)], int(g['num_points']))


def test_fixture_meets_its_condition(golden):
    g = golden('g12_s3dis_sampler.npz')
    k = int(g['num_points'])
    sizes = [g['cloud%d' % c].shape[0] for c in range(3)]
    drawn = [int(g['d%d_cloud' % i][0]) for i in range(N_DRAWS)]
    small = [c for c in drawn if sizes[c] < k]
    assert len(small) >= 2 and sum(sizes[c] >= k for c in drawn) >= 2
    assert any(small.count(c) >= 2 for c in set(small))
    assert sorted(-(-k // s) for s in sizes if s < k) == [2, 4]          # padding with 2 and with 4 permutations


def test_restatement_reproduces_the_reference_fixture(golden):
    g = golden('g12_s3dis_sampler.npz')
    tw = twin_of(g)
    for i in range(N_DRAWS):
        tag = 'd%d_' % i
        d = tw.draw(g[tag + 'noise'], g[tag + 'shuffle'], g[tag + 'choice'])
        assert d['cloud'] == int(g[tag + 'cloud'][0]), i
        assert np.array_equal(d['point_idx'], g[tag + 'point_idx']), i
        assert np.array_equal(d['pos'], g[tag + 'pos']) and d['pos'].dtype == np.float32, i
        assert np.array_equal(d['x'], g[tag + 'x']), i
        assert np.array_equal(d['y'], g[tag + 'y']), i
        assert np.array_equal(np.array(tw.min_possibility), g[tag + 'min_possibility']), i
    for c in range(3):
        assert np.array_equal(tw.possibility[c], g['possibility%d' % c]), c


@pytest.mark.parametrize('k,kc', [(1500, 1000), (1500, 400), (1500, 1499), (1500, 1), (1500, 750), (40960, 15000), (64, 63)])
def test_padding_blocks_are_permutations_and_multiplicities_differ_by_one(k, kc):
    B = 3
    d = PossibilitySampler.draws(77, 5, B, k=k, kc=[kc] * B)
    assert d['choice'].shape == (B, k) and d['choice'].dtype == np.int64 and d['perm'].shape == (B, k)
    nblocks = -(-k // kc)
    for b in range(B):
        assert np.array_equal(np.sort(d['perm'][b, :kc]), np.arange(kc)) and np.all(d['perm'][b, kc:] == -1)
        ch = d['choice'][b]
        for j in range(nblocks - 1):
            assert np.array_equal(np.sort(ch[j * kc:(j + 1) * kc]), np.arange(kc)), (b, j)
        tail = ch[(nblocks - 1) * kc:]
        assert np.unique(tail).size == tail.size and tail.min() >= 0 and tail.max() < kc
        mult = np.bincount(ch, minlength=kc)
        assert mult.min() >= k // kc and mult.max() <= -(-k // kc), (mult.min(), mult.max())
    if kc > 2:
        assert not np.array_equal(d['choice'][0], d['choice'][1])
    again = PossibilitySampler.draws(77, 5, B, k=k, kc=[kc] * B)
    assert np.array_equal(again['choice'], d['choice']) and np.array_equal(again['perm'], d['perm'])


def test_identity_when_the_crop_is_full():
    k = 1500
    d = PossibilitySampler.draws(77, 5, 2, k=k, kc=[k, 600])
    assert np.array_equal(d['choice'][0], np.arange(k))
    assert not np.array_equal(d['choice'][1], np.arange(k))
    # for k_c == k the shuffle is the one the existing form draws, bit for bit; a smaller crop ranks the first k_c hashes of the same row
    plain = PossibilitySampler.draws(77, 5, 2, k=k)
    assert 'choice' not in plain
    assert np.array_equal(d['perm'][0], plain['perm'][0])
    assert np.array_equal(d['perm'][1, :600], plain['perm'][1][plain['perm'][1] < 600])
    for name in ('u', 'normal', 'noise'):
        assert np.array_equal(d[name], plain[name])


def test_numpy_vote_with_repeats_keeps_the_last_row_from_old_values():
    table = np.full((4, 2), 0.5, np.float32)
    visits = np.zeros(4, np.int32)
    probs = np.array([[1, 0], [0, 1], [0.25, 0.75]], np.float32)
    vote_repeated(table, visits, np.array([2, 0, 2]), probs, 0.95)
    s, o = np.float32(0.95), np.float32(1 - 0.95)
    assert np.array_equal(table[2], s * np.float32(0.5) + o * probs[2])            # the last row, formed from the OLD 0.5
    assert np.array_equal(table[0], s * np.float32(0.5) + o * probs[1])
    assert np.array_equal(visits, [1, 0, 1, 0])


def test_form_argument_checks():
    pts = [torch.zeros(10, 3)]
    with pytest.raises(ValueError, match='class_weight'):
        PossibilitySampler(pts, num_points=4, class_weight=np.ones(3), form='s3dis')
    with pytest.raises(ValueError, match='label_to_idx'):
        PossibilitySampler(pts, num_points=4, label_to_idx={1: 0}, form='s3dis')
    with pytest.raises(ValueError, match='form'):
        PossibilitySampler(pts, num_points=4, form='kitti')
    with pytest.raises(ValueError, match='kc'):
        PossibilitySampler.draws(1, 1, 2, k=10, kc=[5])
    with pytest.raises(ValueError, match='kc'):
        PossibilitySampler.draws(1, 1, 1, k=10, kc=[11])
    with pytest.raises(_lib.CrfConvError, match='allow_repeats'):
        VoteAccumulator([4], 2, device='cpu').update(torch.zeros((1, 2), dtype=torch.int64), [0], probs=torch.zeros(2, 2), repeated=True)


def test_entry_points_are_registered_and_declared():
    header = open(os.path.join(ROOT, 'include', 'crfconv_amd.h')).read()
    for name in ('crfconv_possibility_crop_batch_s3dis', 'crfconv_possibility_crop_batch_s3dis_workspace', 'crfconv_vote_update_repeated'):
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\(' % name, header), name
    for name in ('crfconv_possibility_crop_batch_s3dis', 'crfconv_vote_update_repeated'):
        decl = re.search(r'int %s\((.*?)\);' % name, header, re.S).group(1)
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
