"""The Python side of the C ABI is read from include/crfconv_amd.h (crfconv_amd._lib.parse_header): the record layouts agree with the
host C compiler's, the type map is pinned, and a declaration outside the header's dialect is refused, never skipped.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from abi_counts import N_FUNCTIONS, N_RECORDS
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'crfconv_amd.h')


@pytest.fixture(scope='module')
def parsed():
    with open(HEADER) as f:
        return _lib.parse_header(f.read())


def test_record_layout_matches_the_compiler(parsed, tmp_path):
    cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
    if cc is None:
        pytest.skip('no C compiler on PATH')
    _, records = parsed
    assert len(records) == N_RECORDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crfconv_amd.h"', 'int main(void) {']
    for name, fields in records.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f, _ in fields]
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    compiled = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    derived = {}
    for name, fields in records.items():
        cls = getattr(_lib, _lib.record_class_name(name))
        assert cls is _lib.RECORDS[name] and [f for f, _ in cls._fields_] == [f for f, _ in fields]
        derived[name] = str(ctypes.sizeof(cls))
        derived.update(('%s.%s' % (name, f), str(getattr(cls, f).offset)) for f, _ in fields)
    assert len(derived) == N_RECORDS + sum(len(f) for f in records.values())
    assert derived == compiled, {k: (derived.get(k), compiled.get(k)) for k in set(derived) | set(compiled)
                                 if derived.get(k) != compiled.get(k)}


def _parameters(name):
    """[(type text, parameter name)] of a prototype, read from the raw header independently of parse_header."""
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    params = re.search(r'\b%s\s*\(([^()]*)\)' % name, text).group(1)
    return [] if params.strip() == 'void' else [re.fullmatch(r'\s*(.*?)(\w+)\s*', p, re.S).groups() for p in params.split(',')]


def test_type_map_is_pinned(parsed):
    functions, records = parsed
    assert functions == _lib.SIGNATURES
    assert len(_lib.SIGNATURES) == N_FUNCTIONS and len(_lib.RECORDS) == N_RECORDS
    assert _lib.SIGNATURES['crfconv_last_error'] == (ctypes.c_char_p, [])
    assert _lib.SIGNATURES['crfconv_grid_subsample'][0] is ctypes.c_int64
    assert _lib.SIGNATURES['crfconv_pointconv_workspace'][0] is ctypes.c_size_t
    assert _lib.SIGNATURES['crfconv_pointconv_combine'][1][6] is ctypes.c_double
    seed = [n for _, n in _parameters('crfconv_augment')].index('seed')
    assert _lib.SIGNATURES['crfconv_augment'][1][seed] is ctypes.c_uint64
    pointers = 0
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        params = _parameters(name)
        assert len(params) == len(argtypes), name
        for (ctext, pname), argtype in zip(params, argtypes):
            if '*' in ctext or ctext.split() == ['crf_stream_t']:
                assert argtype is ctypes.c_void_p, (name, pname)
                pointers += 1
            else:
                assert argtype is not ctypes.c_void_p, (name, pname)
    assert pointers
    assert ('pad_', ctypes.c_int32) in _lib.Fold1BwdJob._fields_
    for c_name, py_name in (('crf_reduce_job', 'ReduceJob'), ('crf_pc_dump_job', 'PcDumpJob'), ('crf_reduce64_job', 'Reduce64Job'),
                            ('crf_fold1_bwd_job', 'Fold1BwdJob'), ('crf_uv_fold', 'UvFold'), ('crf_augment_spec', 'AugmentSpec')):
        assert _lib.RECORDS[c_name] is getattr(_lib, py_name) and issubclass(getattr(_lib, py_name), ctypes.Structure)


@pytest.mark.parametrize('text, named', [
    ('typedef struct { int a; long double x; } crf_t;', 'crf_t'),                       # a type outside the map, in a record
    ('int crfconv_f(long double x);', 'crfconv_f'),                                     # and in a prototype
    ('int crfconv_f(crf_missing_job job);', 'crfconv_f'),                               # an undeclared record by value
    ('int crfconv_a(void);\nstray\nint crfconv_b(int n);', 'stray'),                    # a stray token between two prototypes
    ('int crfconv_a(void);\nint crfconv_b(int n);\nstray', 'stray'),                    # and after the last one
    ('int crfconv_a(void);\nint crfconv_table[4];', 'crfconv_table'),                   # not a prototype
    ('typedef struct { int a[4]; } crf_t;', 'crf_t'),                                   # an array field
    ('int crfconv_a(int);', 'crfconv_a'),                                               # an unnamed parameter
])
def test_parse_header_refuses_what_it_does_not_understand(text, named):
    good = 'typedef void* crf_stream_t;\nenum { CRF_OK = 0 };\nint crfconv_ok(const float* const* x, crf_stream_t stream);\n'
    functions, records = _lib.parse_header(good)
    assert functions == {'crfconv_ok': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])} and records == {}
    with pytest.raises(_lib.CrfConvError, match=named):
        _lib.parse_header(good + text)


def test_device_descriptor_rows_are_int64_words():
    """sampling.py writes crf_cloud_desc / crf_vote_desc tables as torch.int64 rows, one 8-byte word per field, in this order."""
    for cls, names in ((_lib.CloudDesc, ['points', 'possibility', 'point_weight', 'labels', 'rgb', 'n']),
                       (_lib.VoteDesc, ['test_probs', 'visits', 'last_row', 'n'])):
        assert [f for f, _ in cls._fields_] == names
        assert all(ctypes.sizeof(t) == 8 for _, t in cls._fields_)
        assert [getattr(cls, f).offset for f in names] == [8 * i for i in range(len(names))] and ctypes.sizeof(cls) == 8 * len(names)
