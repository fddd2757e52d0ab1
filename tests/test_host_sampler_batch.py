"""No GPU: the host twin of the batched crop sampler's draws (sampling.PossibilitySampler.draws, csrc/sampler.hip smp_hash) and the
registration of its entry point."""
import os
import re

import numpy as np

from crfconv_amd import _lib
from crfconv_amd.sampling import PossibilitySampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draws_are_a_function_of_seed_counter_and_crop():
    a = PossibilitySampler.draws(1234, 7, 4, k=500, noise_scale=0.35)
    b = PossibilitySampler.draws(1234, 7, 4, k=500, noise_scale=0.35)
    for name in ('u', 'normal', 'noise', 'perm'):
        assert np.array_equal(a[name], b[name]), name
    assert a['u'].shape == (4, 3, 2) and a['noise'].shape == (4, 3) and a['perm'].shape == (4, 500)
    assert a['perm'].dtype == np.int64
    assert np.all(a['u'] > 0) and np.all(a['u'] <= 1)
    assert np.array_equal(a['noise'], a['normal'] * 0.35)
    other_counter = PossibilitySampler.draws(1234, 8, 4, k=500)
    other_seed = PossibilitySampler.draws(1235, 7, 4, k=500)
    for o in (other_counter, other_seed):
        assert not np.array_equal(o['u'], a['u']) and not np.array_equal(o['perm'], a['perm'])
    for i in range(4):                                   # the crops of one call draw apart
        for j in range(i + 1, 4):
            assert not np.array_equal(a['u'][i], a['u'][j]) and not np.array_equal(a['perm'][i], a['perm'][j])
    # a larger batch repeats the crops it shares with a smaller one (keyed on b, not on B)
    assert np.array_equal(PossibilitySampler.draws(1234, 7, 2, k=500)['perm'], a['perm'][:2])


def test_every_shuffle_is_a_permutation():
    for k in (1, 2, 63, 1500, 40960):
        perm = PossibilitySampler.draws(99, 3, 3, k=k)['perm']
        for b in range(3):
            assert np.array_equal(np.sort(perm[b]), np.arange(k)), (k, b)
    assert not np.array_equal(PossibilitySampler.draws(99, 3, 1, k=1500)['perm'][0], np.arange(1500))


def test_normals_have_mean_zero_and_variance_one():
    """4096 x 3 standard normals: the sample mean has standard error 1 / sqrt(n), the sample variance sqrt(2 / n); both within
    5 standard errors (derived bounds)."""
    v = PossibilitySampler.draws(2024, 1, 4096)['normal'].ravel()
    n = v.size
    assert n == 4096 * 3
    assert abs(v.mean()) < 5 / np.sqrt(n), v.mean()
    assert abs(v.var() - 1) < 5 * np.sqrt(2 / n), v.var()
    assert np.abs(v).max() <= 8.6                        # sqrt(-2 ln 2^-53) = 8.57


def test_entry_point_is_registered_and_declared():
    header = open(os.path.join(ROOT, 'include', 'crfconv_amd.h')).read()
    for name in ('crfconv_possibility_crop_batch', 'crfconv_possibility_crop_batch_workspace'):
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\(' % name, header), name
    assert 'crf_cloud_desc' in header
    # one ctypes argument per parameter of the declaration
    decl = re.search(r'int crfconv_possibility_crop_batch\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES['crfconv_possibility_crop_batch'][1])
    assert 'sampler.hip' in open(os.path.join(ROOT, 'crfconv_amd', 'csrc', 'Makefile')).read()
