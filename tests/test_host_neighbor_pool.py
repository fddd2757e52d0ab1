"""The neighbour pooling family (csrc/pool.hip: crfconv_neighbor_pool_forward / _backward) as far as it goes without a GPU: the two
prototypes took the slots of crfconv_neighbor_maxpool_forward and crfconv_gather_rows_backward (whose callers run the new entries with
reduce = 2 and with K = 1, count = NULL), the header's pinned counts stay, every bad argument is refused before any device work, and
the Python surface exists."""
import ctypes
import inspect
import os

import pytest

from abi_counts import N_FUNCTIONS, N_RECORDS
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'crfconv_amd.h')
CRF_ERR_ARG = -1
OLD = ('crfconv_neighbor_maxpool_forward', 'crfconv_gather_rows_backward')
NEW = ('crfconv_neighbor_pool_forward', 'crfconv_neighbor_pool_backward')


@pytest.fixture(scope='module')
def header():
    with open(HEADER) as f:
        text = f.read()
    return text, _lib.parse_header(text)


def test_header_has_the_two_entries_in_the_place_of_the_two_they_subsume(header):
    text, (functions, records) = header
    v, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    #                                          x  idx32 K  m_tgt C reduce out arg count stream
    assert functions[NEW[0]] == (ctypes.c_int, [v, v, i, l, i, i, v, v, v, v])
    #                                          gout count rev_ptr rev_eid K m_src C dx stream
    assert functions[NEW[1]] == (ctypes.c_int, [v, v, v, v, i, l, i, v, v])
    for name in NEW:
        assert _lib.SIGNATURES[name] == functions[name]
    for name in OLD:
        assert name not in functions and name not in _lib.SIGNATURES and name + '(' not in text
    for kept in ('crfconv_neighbor_maxpool_affine_forward', 'crfconv_neighbor_maxpool_backward', 'crfconv_gather_rows'):
        assert kept in functions
    assert functions['crfconv_neighbor_maxpool_backward'] == (ctypes.c_int, [v, v, v, v, i, l, i, v, v])
    assert functions['crfconv_gather_rows'] == (ctypes.c_int, [v, v, l, i, v, v])
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS
    assert set(_lib.SIGNATURES) == set(functions)


def test_header_declares_the_argument_types_of_the_specification(header):
    """The parsed form above sees every pointer as void*: the element types are read from the text."""
    text = ' '.join(header[0].split())
    assert ('int crfconv_neighbor_pool_forward(const float* x, const int32_t* idx32, int K, int64_t m_tgt, int C, int reduce, '
            'float* out, int32_t* arg, int32_t* count, crf_stream_t stream);') in text
    assert ('int crfconv_neighbor_pool_backward(const float* gout, const int32_t* count, const int32_t* rev_ptr, '
            'const int32_t* rev_eid, int K, int64_t m_src, int C, float* dx, crf_stream_t stream);') in text


def test_library_exports():
    lib = _lib.load()
    for name in NEW + ('crfconv_neighbor_maxpool_affine_forward', 'crfconv_neighbor_maxpool_backward', 'crfconv_gather_rows'):
        assert hasattr(lib, name)
    for name in OLD:
        assert not hasattr(lib, name)


# arguments of a valid call: addresses are never dereferenced by a refused call
X, IDX, OUT, ARG, CNT, GOUT, RPTR, REID, DX = (0x1000 * n for n in range(1, 10))


def forward(x=X, idx=IDX, K=16, m_tgt=10, C=8, reduce=0, out=OUT, arg=ARG, count=CNT):
    return _lib.load().crfconv_neighbor_pool_forward(x, idx, K, m_tgt, C, reduce, out, arg, count, None)


def backward(gout=GOUT, count=CNT, rev_ptr=RPTR, rev_eid=REID, K=16, m_src=10, C=8, dx=DX):
    return _lib.load().crfconv_neighbor_pool_backward(gout, count, rev_ptr, rev_eid, K, m_src, C, dx, None)


@pytest.mark.parametrize('bad', [
    dict(reduce=-1), dict(reduce=4),
    dict(x=None), dict(idx=None), dict(out=None),
    dict(reduce=2, arg=None), dict(reduce=3, arg=None),
    dict(reduce=1, count=None),
    dict(C=6), dict(C=0), dict(K=0), dict(m_tgt=0), dict(m_tgt=-1), dict(m_tgt=1 << 31),
    dict(reduce=4, arg=None, count=None), dict(reduce=2, arg=None, count=None), dict(reduce=1, arg=None, count=None),
], ids=lambda b: ','.join('%s=%s' % kv for kv in b.items()))
def test_forward_refuses_bad_arguments_before_any_device_work(bad):
    assert forward(**bad) == CRF_ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('bad', [
    dict(gout=None), dict(rev_ptr=None), dict(rev_eid=None), dict(dx=None),
    dict(C=6), dict(K=0), dict(m_src=0), dict(m_src=1 << 31),
    dict(count=None, gout=None), dict(K=1, count=None, dx=None),
], ids=lambda b: ','.join('%s=%s' % kv for kv in b.items()))
def test_backward_refuses_bad_arguments_before_any_device_work(bad):
    assert backward(**bad) == CRF_ERR_ARG
    assert _lib.last_error()


def test_python_surface_without_a_gpu():
    import torch
    from crfconv_amd import ops
    from crfconv_amd.models import common
    assert 'neighbor_pool' in ops.__all__ and callable(ops.neighbor_pool)
    assert 'neighbor_maxpool' in ops.__all__ and 'gather_rows' in ops.__all__
    assert inspect.signature(ops.neighbor_pool).parameters['reduce'].default == 'sum'
    assert issubclass(ops._NeighborPool, torch.autograd.Function)
    assert ops.POOL_REDUCE == {'sum': 0, 'add': 0, 'mean': 1, 'max': 2, 'min': 3}
    x = torch.zeros((4, 8))
    for bad in ('prod', 'Sum', None, 2):
        with pytest.raises(ValueError):
            ops.neighbor_pool(x, None, bad)                 # refused before the table or a device is looked at
    for reduce in ('sum', 'add', 'mean', 'max', 'min'):
        with pytest.raises(_lib.CrfConvError, match='no CPU path'):
            ops.neighbor_pool(x, None, reduce)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        common.fps_pooling(torch.zeros((4, 3)), x, torch.zeros((4, 5)))
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):
        common.fps_max_pooling(torch.zeros((4, 3)), x)
    with pytest.raises(ValueError):
        common.fps_pooling(torch.zeros((4, 3)), x, torch.zeros((4, 5)), reduce='min')      # the reference's own list


def test_fps_pooling_helpers_have_the_reference_signatures():
    """models/common.py:9, 18 of the reference: names, order and defaults; ptr is this library's keyword-only addition."""
    from crfconv_amd.models import common

    def spec(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]
    E, PK, KW = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert spec(common.fps_pooling) == [('pos', E, PK), ('x', E, PK), ('edge_attr', E, PK), ('batch', None, PK), ('k', 16, PK),
                                        ('r', 0.5, PK), ('reduce', 'sum', PK), ('ptr', None, KW)]
    assert spec(common.fps_max_pooling) == [('pos', E, PK), ('x', E, PK), ('batch', None, PK), ('k', 16, PK), ('r', 0.5, PK),
                                            ('ptr', None, KW)]
