"""The single kernels and the job forms of the row-streaming kernels include ONE text of statements each (csrc/linear_fwd_body.inc,
mlp_bwd_p1_body.inc).  What a job may never do is read the launch's own coordinates or own LDS: the text reaches both only through what
its includer provides -- the coordinate macros, and for the backward pass the last-workgroup test -- and the single kernels provide the
launch's.  No GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crfconv_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# included text: (the file that includes it, the single kernel's head, the body function's head, what the kernel's macros must say)
BODIES = {
    'linear_fwd_body.inc': ('linear_fwd.hpp', '__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_kernel(',
                            '__device__ __forceinline__ void linear_fwd_body(',
                            {'LF_BX': 'blockIdx.x', 'LF_BY': 'blockIdx.y', 'LF_NBX': 'gridDim.x'}),
    'mlp_bwd_p1_body.inc': ('mlp_bwd.hip', '__global__ __launch_bounds__(WG_BLOCK) void mlp_bwd_p1_kernel(',
                            '__device__ __forceinline__ void mlp_bwd_p1_body(',
                            {'P1_BX': 'blockIdx.x', 'P1_BY': 'blockIdx.y', 'P1_BZ': 'blockIdx.z', 'P1_NBX': 'gridDim.x',
                             'P1_LAST': 'last_workgroup(ticket, gridDim.x * gridDim.y * gridDim.z, &s_flag)'}),
}


def _function(text, head):
    """The definition that starts at `head` (which must occur once), up to the closing brace at the start of a line."""
    assert text.count(head) == 1, head
    a = text.index(head)
    return text[a:text.index('\n}\n', a)]


def test_the_shared_statements_never_read_the_launch():
    """A job's workgroup is not the launch's: the included text names neither the launch's coordinates nor LDS of its own."""
    for inc in BODIES:
        assert not re.search(r'blockIdx|gridDim|__shared__', _read(inc)), inc


def test_each_text_is_included_by_its_kernel_and_its_body_function():
    for inc, (host, kernel, body, _) in BODIES.items():
        line = '#include "%s"' % inc
        counts = {name: _read(name).count(line) for name in sorted(os.listdir(CSRC)) if name.endswith(('.hip', '.hpp', '.h', '.inc'))}
        assert {n: c for n, c in counts.items() if c} == {host: 2}, (inc, counts)
        text = _read(host)
        assert _function(text, kernel).count(line) == 1 and _function(text, body).count(line) == 1, inc


def test_the_kernels_provide_the_launchs_own_coordinates():
    """The single kernel's macros are the launch's coordinates and the whole-grid last-workgroup test; the body function defines the same
    names from its arguments, and neither lets a macro outlive the include."""
    for inc, (host, kernel, body, want) in BODIES.items():
        text = _read(host)
        for head in (kernel, body):
            fn = _function(text, head)
            defines = dict(re.findall(r'^#define (\w+) (.*)$', fn, re.M))
            assert set(defines) == set(want), (inc, head, defines)
            assert sorted(re.findall(r'^#undef (\w+)$', fn, re.M)) == sorted(want), (inc, head)
            if head == kernel:
                assert defines == want, (inc, defines)
            else:
                assert not re.search(r'blockIdx|gridDim', fn), (inc, head)


def test_internal_job_records_match_the_compiler(tmp_path):
    """csrc/stream_jobs.h -- the entries only the package calls -- is read by the same parser into tables of its own: the public tables hold
    none of its names, and the ctypes layout of its records is the host C compiler's."""
    import ctypes
    import shutil
    import subprocess

    from crfconv_amd import _lib
    assert set(_lib.INTERNAL_RECORDS) == {'crf_linear_job', 'crf_mlp_stream_bwd_job'}
    assert not set(_lib.INTERNAL_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.INTERNAL_RECORDS) & set(_lib.RECORDS)
    assert _lib.INTERNAL_RECORDS['crf_linear_job'] is _lib.LinearJob and _lib.INTERNAL_RECORDS['crf_mlp_stream_bwd_job'] is _lib.MlpStreamBwdJob
    assert all(res is ctypes.c_int for res, _ in _lib.INTERNAL_SIGNATURES.values())
    cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
    assert cc is not None, 'no C compiler on PATH'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stream_jobs.h"', 'int main(void) {']
    for name, cls in _lib.INTERNAL_RECORDS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f, _ in cls._fields_]
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)])
    compiled = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    derived = {}
    for name, cls in _lib.INTERNAL_RECORDS.items():
        derived[name] = str(ctypes.sizeof(cls))
        derived.update(('%s.%s' % (name, f), str(getattr(cls, f).offset)) for f, _ in cls._fields_)
    assert derived == compiled
