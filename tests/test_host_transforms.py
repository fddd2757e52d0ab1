"""CPU checks of crfconv_amd.transforms: the host twin of the per-cloud augmentation draws (Compose.draws) and its laws, the
validation of the chain, the seeding.  No GPU and no library needed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from crfconv_amd import transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def train_chain(generator=None, **kw):
    """trainval.py:26-36 as written."""
    return T.Compose([
        T.RandomRotate(degrees=180, axis=2),
        T.RandomScaleAnisotropic(scales=[0.8, 1.2], anisotropic=True),
        T.RandomSymmetry(axis=[True, False, False]),
        T.RandomNoise(sigma=0.001),
        T.DropFeature(drop_proba=0.2, feature_name='rgb'),
        T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'rgb'], delete_feats=[False, True]),
    ], generator=generator, **kw)


def test_draws_are_a_function_of_seed_counter_and_cloud():
    c = train_chain(torch.Generator().manual_seed(0))
    a, b = c.draws(1234, 7, 16), c.draws(1234, 7, 16)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    more = c.draws(1234, 7, 40)                          # cloud b's draws do not depend on the batch size
    np.testing.assert_array_equal(more['u'][:16], a['u'])
    other = c.draws(1234, 8, 16)                         # the next counter: new draws for every cloud
    assert np.all(np.any(other['u'] != a['u'], axis=1))
    assert np.all(np.any(c.draws(1235, 7, 16)['u'] != a['u'], axis=1))
    assert a['u'].dtype == np.float32 and np.all((a['u'] >= 0) & (a['u'] < 1))
    np.testing.assert_array_equal(a['u'] * np.float32(2 ** 24), np.floor(a['u'] * np.float32(2 ** 24)))      # 24-bit uniforms


def test_draw_laws_over_ten_thousand_clouds():
    n = 10000
    c = train_chain(torch.Generator().manual_seed(1))
    d = c.draws(987654321, 3, n)
    # theta ~ U(-pi, pi): Kolmogorov-Smirnov statistic below its alpha = 1e-3 critical value
    th = np.sort(d['theta'])
    assert th.min() >= -np.pi and th.max() <= np.pi
    cdf = (th + np.pi) / (2 * np.pi)
    i = np.arange(1, n + 1)
    ks = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    crit = np.sqrt(-0.5 * np.log(1e-3 / 2)) / np.sqrt(n)
    assert ks < crit, (ks, crit)
    np.testing.assert_allclose(d['cos'], np.cos(d['theta']), atol=1e-7)
    np.testing.assert_allclose(d['sin'], np.sin(d['theta']), atol=1e-7)
    # scales in [0.8, 1.2], mean within 4 sigma of 1.0, per axis
    s = d['scale']
    assert s.min() >= np.float32(0.8) and s.max() <= np.float32(1.2)
    sig = 0.4 / np.sqrt(12) / np.sqrt(n)
    assert np.all(np.abs(s.mean(0) - 1.0) < 4 * sig), s.mean(0)
    # flips: x only (RandomSymmetry(axis=[True, False, False])), rate 1/2
    assert np.all((d['flip'] & ~1) == 0)
    rate = (d['flip'] & 1).mean()
    assert abs(rate - 0.5) < 4 * np.sqrt(0.25 / n), rate
    # the crop's rgb is dropped with probability 0.2
    drop = 1.0 - d['keep'].mean()
    assert abs(drop - 0.2) < 4 * np.sqrt(0.2 * 0.8 / n), drop
    # independence of the parameters of one cloud (different hash slots)
    corr = np.corrcoef(d['u'].T)
    assert np.all(np.abs(corr - np.eye(8)) < 4 / np.sqrt(n))
    # params: the kernel's params_out layout
    p = d['params']
    np.testing.assert_array_equal(p[:, 0], d['cos'])
    np.testing.assert_array_equal(p[:, 2:5], s)
    np.testing.assert_array_equal(p[:, 5], d['flip'])
    np.testing.assert_array_equal(p[:, 6], d['keep'])


def test_other_axes_and_ranges():
    c = T.Compose([T.RandomRotate(degrees=(10, 20), axis=0), T.RandomSymmetry(axis=[False, True, True])],
                  generator=torch.Generator().manual_seed(2))
    d = c.draws(5, 0, 4000)
    deg = np.degrees(d['theta'])
    assert deg.min() >= 10 and deg.max() < 20
    assert np.all((d['flip'] & 1) == 0) and 0.4 < (d['flip'] & 2).mean() / 2 < 0.6 and 0.4 < (d['flip'] & 4).mean() / 4 < 0.6
    np.testing.assert_array_equal(d['scale'], 1.0)       # steps the chain lacks are the identity
    assert d['keep'].all()


def test_unsupported_chains_are_rejected():
    ok = [T.RandomRotate(180, axis=2), T.RandomNoise(0.01)]
    T.Compose(ok)
    with pytest.raises(NotImplementedError, match='RandomRotate'):
        T.Compose(ok[::-1])                              # another order
    with pytest.raises(NotImplementedError, match='RandomNoise'):
        T.Compose([T.RandomNoise(0.01), T.RandomNoise(0.02)])
    with pytest.raises(NotImplementedError, match='RandomScaleAnisotropic'):
        T.Compose([T.AddFeatsByKeys([True], ['pos']), T.RandomScaleAnisotropic([0.9, 1.1])])     # AddFeatsByKeys must come last

    class Jitter:
        pass
    with pytest.raises(NotImplementedError, match='Jitter'):
        T.Compose([T.RandomRotate(30, axis=2), Jitter()])
    with pytest.raises(NotImplementedError, match="'norm'"):
        T.Compose([T.DropFeature(0.2, feature_name='norm')])
    with pytest.raises(NotImplementedError, match="'norm'"):
        T.Compose([T.AddFeatsByKeys([True, True], ['pos', 'norm'])])
    with pytest.raises(NotImplementedError, match='pos cannot be deleted'):
        T.Compose([T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[True, False])])
    with pytest.raises(NotImplementedError, match='AddFeatsByKeys'):
        T.Compose([T.AddFeatsByKeys([True, True], ['rgb', 'pos'])])              # x must be [pos, rgb]
    with pytest.raises(NotImplementedError, match='norm'):                       # a norm field on the data (checked before any device work)
        from crfconv_amd.data import Data
        train_chain()(Data(pos=torch.zeros(4, 3), rgb=torch.zeros(4, 3), norm=torch.zeros(4, 3)))
    with pytest.raises(ValueError):
        T.RandomRotate(30, axis=3)
    with pytest.raises(ValueError):
        T.RandomScaleAnisotropic([1.2, 0.8])
    # the validation chain of trainval.py:37-42 and a lone transform are fine
    T.Compose([T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'rgb'], delete_feats=[False, True])])
    T.Compose([T.RandomSymmetry(axis=[True, False, False])])


def test_seeding_and_state():
    g = torch.Generator().manual_seed(11)
    a, b = train_chain(g), train_chain(g)
    assert a.seed != b.seed                               # one draw per Compose on the caller's generator
    assert train_chain(torch.Generator().manual_seed(11)).seed == a.seed
    before = torch.get_rng_state()
    train_chain()                                         # no generator: the global one does not advance
    assert torch.equal(before, torch.get_rng_state())
    sd = a.state_dict()
    assert sd == {'seed': a.seed, 'counter': 0}
    b.load_state_dict({'seed': 42, 'counter': 9})
    assert b.state_dict() == {'seed': 42, 'counter': 9}


def test_construction_and_draws_do_not_load_the_library():
    code = ('import crfconv_amd.transforms as T, crfconv_amd._lib as L\n'
            'c = T.Compose([T.RandomRotate(180, axis=2), T.RandomSymmetry([True, False, False]), T.DropFeature(0.2)])\n'
            'c.draws(1, 2, 3); c.state_dict()\n'
            'assert L._lib is None\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
