"""The dilated table-finishing entry (csrc/graph_table.hip: crfconv_graph_table_dilated) as far as it goes without a GPU: its
prototype took the slot of the single-layer crfconv_crf_matrices (whose caller runs the batched entry with one job), the header's pinned
counts stay, every bad argument is refused before any device work, the Python surface exists, and the numpy restatement the GPU tests
compare with has the properties of the specification."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from abi_counts import N_FUNCTIONS, N_RECORDS
import dilated_restatement as R
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'crfconv_amd.h')
CRF_OK, CRF_ERR_ARG = 0, -1
SEED = 20250                # the seed of the uniformity case, here and in test_gpu_dilated_table.py


@pytest.fixture(scope='module')
def header():
    with open(HEADER) as f:
        text = f.read()
    return text, _lib.parse_header(text)


def test_header_has_the_entry_in_the_place_of_the_single_layer_matrices(header):
    text, (functions, records) = header
    restype, argtypes = functions['crfconv_graph_table_dilated']
    v, i, l, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    assert restype is ctypes.c_int and argtypes == [v, l, i, l, i, u64, v, l, i, v, i, v, v]
    assert _lib.SIGNATURES['crfconv_graph_table_dilated'] == (restype, argtypes)
    assert 'crfconv_crf_matrices' not in functions and 'crfconv_crf_matrices(' not in text
    assert 'crfconv_crf_matrices_batched' in functions and 'crfconv_crf_matrices_backward' in functions
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS


def test_library_exports():
    lib = _lib.load()
    assert hasattr(lib, 'crfconv_graph_table_dilated') and hasattr(lib, 'crfconv_crf_matrices_batched')
    assert not hasattr(lib, 'crfconv_crf_matrices')


# arguments of a valid call: addresses are never dereferenced by a refused call (nor by n_tgt = 0, which launches nothing)
NBR, OUT, CNT, CTR = 0x1000, 0x2000, 0x3000, 0x4000


def call(nbr=NBR, n_tgt=10, K=32, n_src=10, k=16, seed=7, counter=CTR, salt=0, mode=0, out=OUT, K_out=None, counts=CNT):
    K_out = k + (mode == 2) if K_out is None else K_out
    return _lib.load().crfconv_graph_table_dilated(nbr, n_tgt, K, n_src, k, seed, counter, salt, mode, out, K_out, counts, None)


@pytest.mark.parametrize('bad', [
    dict(nbr=None), dict(out=None), dict(counts=None), dict(counter=None), dict(out=NBR),
    dict(K=0), dict(K=65), dict(k=0), dict(k=65),
    dict(mode=-1), dict(mode=3),
    dict(K_out=17), dict(mode=2, K_out=16), dict(mode=1, K_out=17), dict(k=64, mode=2), dict(k=64, mode=2, K_out=64),
    dict(mode=1, n_src=11), dict(mode=2, n_src=9),
    dict(n_tgt=-1), dict(n_src=-1),
    dict(n_tgt=1 << 27, n_src=1 << 27), dict(salt=-1),
])
def test_bad_arguments_are_refused_before_any_device_work(bad):
    assert call(**bad) == CRF_ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_no_rows_is_no_launch(mode):
    assert call(n_tgt=0, n_src=0, mode=mode) == CRF_OK
    assert call(n_tgt=0, n_src=0, mode=mode, K=64, k=63, seed=(1 << 64) - 1, salt=(1 << 62)) == CRF_OK
    assert call(n_tgt=0, n_src=7, mode=0, K=1, k=1) == CRF_OK


def test_python_surface_without_a_gpu():
    import torch
    from crfconv_amd import graph
    from crfconv_amd.models import graph_ops, point_conv
    for name in ('DilationDraw', 'knn_dilated_table', 'knn_dilated'):
        assert callable(getattr(graph_ops, name))
    assert callable(point_conv.use_device_dilation)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        graph.table_from_search_dilated(torch.zeros((4, 3), dtype=torch.int32), 4, 2, seed=1, counter=torch.zeros(1, dtype=torch.int64),
                                        salt=0)
    assert point_conv._SparseEncoder.dilation_draw is None and point_conv._SparseEncoder.graph_tables is False
    assert inspect.signature(point_conv.build_graph).parameters['draw'].default is None
    assert inspect.signature(point_conv.build_bipartite_graph).parameters['draw'].default is None
    assert inspect.signature(graph.table_from_search_dilated).parameters['read_counts'].default is True
    draw = graph_ops.DilationDraw(5, 'cpu')
    assert [draw.salt() for _ in range(4)] == [0, 1, 2, 3] and draw.seed == 5
    assert draw.counter.dtype == torch.int64 and draw.counter.tolist() == [0]
    assert draw.step() is draw and draw.counter.tolist() == [1] and draw.salt() == 4
    # the device draw makes tables only, and the search has 64 columns: both refused before anything touches a device
    pos = torch.zeros((8, 3))
    with pytest.raises(ValueError):
        point_conv.build_graph(pos, None, method='knn', k=2, dilation=2, draw=draw)
    with pytest.raises(ValueError):
        point_conv.build_bipartite_graph(pos, None, 0.5, method='knn', k=2, dilation=2, draw=draw)
    with pytest.raises(ValueError):
        graph_ops.knn_dilated_table(pos, pos, 13, 5, draw=draw)


# ------------------------------------------------------------------------------------------ the restatement's own properties
def test_restatement_hash_is_the_specified_one():
    """One value worked out by hand in Python integers, mod 2^64."""
    seed, counter, salt, i, t = 0x0123456789ABCDEF, 3, 5, 1000, 7
    m = (1 << 64) - 1
    z = ((seed ^ 0xA0761D6478BD642F) + 0x9E3779B97F4A7C15 * (counter + 1) + salt * 0xC2B2AE3D27D4EB4F + (i * 64 + t) * 0xD1B54A32D192ED03) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    h = z ^ (z >> 31)
    got = R.hashes(R.key_of(seed, counter, salt), np.array([i * 64 + t], dtype=np.uint64))
    assert int(got[0]) == h
    assert int(R.slots_of(R.key_of(seed, counter, salt), [i], 8, 37)[0, 7]) == ((h >> 32) * 37) >> 32


def holes(n, K, n_src, seed):
    """[n, K] entries of [0, n_src) with -1 and n_src + 3 anywhere, every seventh row empty, row 1 with one entry."""
    rng = np.random.default_rng(seed)
    tab = rng.integers(0, n_src, (n, K)).astype(np.int32)
    u = rng.random((n, K))
    tab[u < 0.3] = -1
    tab[(u >= 0.3) & (u < 0.4)] = n_src + 3
    tab[np.arange(n) % 7 == 3] = -1
    if n > 1:
        tab[1] = -1
        tab[1, K - 1] = 0
    return tab


@pytest.mark.parametrize('K,k', [(3, 2), (17, 4), (64, 16), (64, 63)])
def test_restatement_picks_are_valid_entries_and_counted(K, k):
    n, n_src = 200, 150
    tab = holes(n, K, n_src, 11 * K + k)
    for mode in (0, 1, 2):
        ns = n if mode else n_src
        picks, row, col = R.dilate(tab, ns, k, seed=9, counter=2, salt=4, self_mode=mode)
        assert len(picks) == n
        for i, p in enumerate(picks):
            valid = tab[i][(tab[i] >= 0) & (tab[i] < ns)]
            assert p.size == min(k, valid.size)                       # n_pick = min(k, have)
            assert np.isin(p, valid).all()                            # every pick is a valid entry of its row
        kept = sum(int((p != i).sum()) if mode else p.size for i, p in enumerate(picks))
        assert row.size == col.size == kept + (n if mode == 2 else 0)
        assert (np.diff(row[:kept]) >= 0).all()                       # row-major
        if mode:
            assert (row[:kept] != col[:kept]).all()
        if mode == 2:
            assert np.array_equal(row[kept:], np.arange(n)) and np.array_equal(col[kept:], np.arange(n))
    # another counter, salt or seed: other picks
    base = np.concatenate(R.picks_of(tab, n_src, k, 9, 2, 4))
    for other in ((10, 2, 4), (9, 3, 4), (9, 2, 5)):
        assert not np.array_equal(base, np.concatenate(R.picks_of(tab, n_src, k, *other)))


def test_restatement_slots_are_uniform():
    """4096 rows x 16 picks over have = 64: every slot's count within 6 standard deviations of 65536 / 64 = 1024, i.e. within
    6 sqrt(65536 (1/64) (63/64)) = 190.5 -- for the fixed seed (deterministic: the hash has no other input)."""
    slots = R.slots_of(R.key_of(SEED, 0, 0), np.arange(4096), 16, 64)
    assert slots.shape == (4096, 16) and slots.min() >= 0 and slots.max() <= 63
    count = np.bincount(slots.ravel(), minlength=64)
    bound = 6.0 * np.sqrt(65536 * (1 / 64) * (63 / 64))
    assert np.abs(count - 1024).max() <= bound, (count.min(), count.max(), bound)
