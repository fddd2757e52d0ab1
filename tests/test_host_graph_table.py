"""The C ABI of the table-finishing kernel (csrc/graph_table.hip) as far as it goes without a GPU: its prototype took the slot of the
single-table narrowing entry, the header's pinned counts stay, and every bad argument is refused before any device work."""
import ctypes
import os

import pytest

from abi_counts import N_FUNCTIONS, N_RECORDS
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'crfconv_amd.h')
CRF_OK, CRF_ERR_ARG = 0, -1


@pytest.fixture(scope='module')
def header():
    with open(HEADER) as f:
        text = f.read()
    return text, _lib.parse_header(text)


def test_header_has_the_entry_in_the_place_of_the_single_narrowing(header):
    text, (functions, records) = header
    restype, argtypes = functions['crfconv_graph_table']
    v, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert restype is ctypes.c_int and argtypes == [v, l, i, l, v, v, f, i, v, i, v, v]
    assert _lib.SIGNATURES['crfconv_graph_table'] == (restype, argtypes)
    assert 'crfconv_index_narrow_sorted' not in functions and 'crfconv_index_narrow_sorted' not in text
    assert 'crfconv_index_narrow_batched' in functions and 'crf_narrow_job' in records
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS


def test_library_exports():
    lib = _lib.load()
    assert hasattr(lib, 'crfconv_graph_table') and not hasattr(lib, 'crfconv_index_narrow_sorted')


# arguments of a valid call: addresses are never dereferenced by a refused call (nor by n_tgt = 0, which launches nothing)
NBR, OUT, CNT, PS, PT = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000


def call(nbr=NBR, n_tgt=10, K=16, n_src=10, pos_src=None, pos_tgt=None, r2=-1.0, mode=0, out=OUT, K_out=None, counts=CNT):
    K_out = K + (mode == 2) if K_out is None else K_out
    return _lib.load().crfconv_graph_table(nbr, n_tgt, K, n_src, pos_src, pos_tgt, r2, mode, out, K_out, counts, None)


@pytest.mark.parametrize('bad', [
    dict(nbr=None), dict(out=None), dict(counts=None),
    dict(K=0), dict(K=65),
    dict(K_out=17), dict(mode=2, K_out=16), dict(mode=1, K_out=17),
    dict(mode=1, n_src=11), dict(mode=2, n_src=9),
    dict(r2=0.25), dict(r2=0.0, pos_src=PS), dict(r2=0.25, pos_tgt=PT),
    dict(mode=3), dict(out=NBR), dict(n_tgt=1 << 27, n_src=1 << 27),
])
def test_bad_arguments_are_refused_before_any_device_work(bad):
    assert call(**bad) == CRF_ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_no_rows_is_no_launch(mode):
    assert call(n_tgt=0, n_src=0, mode=mode) == CRF_OK
    assert call(n_tgt=0, n_src=0, mode=mode, K=64, r2=1.0, pos_src=PS, pos_tgt=PT) == CRF_OK
    assert call(n_tgt=0, n_src=7, mode=0, K=1) == CRF_OK


def test_python_surface_without_a_gpu():
    import torch
    from crfconv_amd import graph, ops
    from crfconv_amd.models import graph_ops, point_conv
    assert ops.state.no_graph_tables is False
    for name in ('knn_table', 'knn_graph_table', 'radius_graph_table'):
        assert callable(getattr(graph_ops, name))
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        graph.table_from_search(torch.zeros((4, 3), dtype=torch.int32), 4)
    assert point_conv._SparseEncoder.graph_tables is False
    import inspect
    assert inspect.signature(point_conv.build_graph).parameters['as_table'].default is False
    assert inspect.signature(point_conv.build_bipartite_graph).parameters['as_table'].default is False
