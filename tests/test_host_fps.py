"""Farthest point sampling as far as it goes without a GPU: the float64 restatement against a plain statement of the definition, the
pick-count expression against math.ceil, the header's pinned counts, and the condition on the GPU test's inputs -- which clouds the
float32 kernel can be held to the restatement's very picks -- so that tests/test_gpu_fps.py cannot hide behind its fixture."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from abi_counts import N_FUNCTIONS, N_RECORDS
import _seeded as S
import fps_restatement as F
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def definition(p, m):
    """The definition, with the whole distance matrix."""
    sel = [0]
    for _ in range(m - 1):
        sel.append(int(np.argmax(((p[:, None] - p[sel][None]) ** 2).sum(-1).min(1))))
    return sel


def test_restatement_is_the_definition():
    p = S.make_cloud(77, 200).astype(np.float64)
    picks, margin = F.np_fps(p, 50)
    assert picks.tolist() == definition(p, 50) and len(set(picks.tolist())) == 50 and margin > 0
    assert F.walk_along(p, picks) == 1.0
    with pytest.raises(AssertionError):                     # a pick that is not a farthest point is seen
        F.walk_along(p, np.r_[picks[:20], picks[5], picks[21:]])
    # ties go to the lower index: on a lattice, and all picks are row 0 of a cloud of one repeated point
    lat = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing='ij'), -1).reshape(-1, 3)
    got, margin = F.np_fps(lat, 6)
    assert got.tolist() == definition(lat, 6) and got[:3].tolist() == [0, 26, 5] and margin == 0.0
    assert F.np_fps(np.ones((50, 3)), 13)[0].tolist() == [0] * 13
    assert F.np_fps(p, 1)[0].tolist() == [0] and F.np_fps(p[:1], 1)[1] == np.inf


@pytest.mark.parametrize('ratio', [0.1, 0.25, 0.375, 0.5])
def test_pick_counts_equal_math_ceil(ratio):
    from crfconv_amd.models import graph_ops
    n = torch.arange(0, 5001, dtype=torch.int64)
    got = graph_ops.pick_counts(n, ratio)
    want = [0 if v == 0 else max(1, math.ceil(ratio * v)) for v in range(5001)]
    assert got.dtype == torch.int64 and got.tolist() == want
    assert got.tolist() == [F.n_picks(v, ratio) for v in range(5001)]


def test_pick_counts_of_an_int_ratio():
    from crfconv_amd.models import graph_ops
    n = torch.tensor([0, 1, 95, 96, 97, 5000], dtype=torch.int64)
    assert graph_ops.pick_counts(n, 96).tolist() == [0, 1, 95, 96, 96, 96]
    assert graph_ops.pick_counts(n, 1.0).tolist() == n.tolist()


def test_header_keeps_its_counts_and_the_prototype():
    with open(os.path.join(ROOT, 'include', 'crfconv_amd.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS
    v, i = ctypes.c_void_p, ctypes.c_int
    assert functions['crfconv_fps'] == (ctypes.c_int, [v, i, v, v, v, v, v, v, v, v])
    assert hasattr(_lib.load(), 'crfconv_fps')


def test_the_kernel_has_a_unit_of_its_own():
    csrc = os.path.join(ROOT, 'crfconv_amd', 'csrc')
    with open(os.path.join(csrc, 'collate.hip')) as f:
        assert 'fps' not in f.read()
    with open(os.path.join(csrc, 'fps.hip')) as f:
        text = f.read()
    assert 'crfconv_fps' in text and text.count('sub_rn(') == 3       # the squared distance is written once


@pytest.fixture(scope='module')
def margins():
    return {len(p): F.np_fps(p, F.n_picks(len(p), F.RATIO))[1] for p in F.ragged_clouds()}


def test_which_clouds_are_held_to_the_exact_picks(margins):
    """The smallest margin between a winner and its runner-up, per cloud of the ragged batch.  Above TOL the kernel must make the
    restatement's picks; the three large clouds have a pick decided by less and get the walk-along only."""
    print({n: '%.2e' % m for n, m in margins.items()})
    assert sorted(margins) == sorted(F.SIZES)
    exact = [n for n in F.SIZES if margins[n] > F.TOL]
    assert exact == F.EXACT and len(exact) >= 5
    assert margins[700] > 2e-5 and margins[300] > 1e-4 and margins[9] > 0.1 and margins[40] > 0.03 and margins[1025] > 6e-5
    assert all(margins[n] < F.TOL for n in (2048, 4097, 8192))


@pytest.mark.parametrize('seed,n,ratio', F.TIER_CASES)
def test_the_other_tiers_clouds_are_exact_too(seed, n, ratio):
    margin = F.np_fps(S.make_cloud(seed, n, box=(2, 1, 1)), ratio)[1]
    print('n = %d, %d picks: smallest margin %.2e' % (n, ratio, margin))
    assert margin > 3e-5
