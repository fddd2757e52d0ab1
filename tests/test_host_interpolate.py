"""The C ABI and the Python surface of the kNN interpolation operator (csrc/interp.hip, ops/interp.py) as far as they go without a GPU:
one new prototype in the place of the block-stamps diagnostic, the header's pinned counts, the exported symbol, no CPU path."""
import ctypes
import os

import pytest
import torch

from abi_counts import N_FUNCTIONS, N_RECORDS
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'crfconv_amd.h')


@pytest.fixture(scope='module')
def header():
    with open(HEADER) as f:
        text = f.read()
    return text, _lib.parse_header(text)


def test_header_declares_one_entry_for_both_directions(header):
    text, (functions, records) = header
    restype, argtypes = functions['crfconv_interpolate']
    assert restype is ctypes.c_int and len(argtypes) == 13
    v, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert argtypes == [v, v, v, v, i, l, l, i, v, v, v, v, v]
    assert _lib.SIGNATURES['crfconv_interpolate'] == (restype, argtypes)
    assert [n for n in functions if 'interp' in n] == ['crfconv_interpolate']
    assert 'knn' not in 'crfconv_interpolate'                           # the builders' tests count library calls named *knn*
    assert 'zero row' in text and 'rev_ptr == NULL' in text             # the comment states the no-neighbour rule and the direction switch


def test_stamps_entry_left_and_the_counts_stay(header):
    text, (functions, records) = header
    assert 'crfconv_meanfield_forward_block_stamps' not in functions and 'forward_block_stamps' not in text
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS
    assert not os.path.exists(os.path.join(ROOT, 'scratch', 'mf_block_stamps.py'))


def test_library_exports_the_entry():
    lib = _lib.load()
    assert hasattr(lib, 'crfconv_interpolate')
    assert not hasattr(lib, 'crfconv_meanfield_forward_block_stamps')


def test_no_cpu_path():
    from crfconv_amd import ops
    from crfconv_amd.graph import NeighborTable, table_from_index
    x, pos_x, pos_y = torch.ones(4, 8), torch.rand(4, 3), torch.rand(6, 3)
    idx = torch.zeros((6, 3), dtype=torch.int32)
    table = NeighborTable.__new__(NeighborTable)                       # what table_from_index would build, had it a device to build it on
    table.B, table.n_tgt, table.n_src, table.K, table.idx32 = 1, 6, 4, 3, idx
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        ops.interpolate(x, pos_x, pos_y, table)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        ops.knn_interpolate(x, pos_x, pos_y, k=3)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        table_from_index(idx, 4)
    assert ops.interpolate is ops.interp.interpolate and 'interpolate' in ops.__all__ and 'knn_interpolate' in ops.__all__
