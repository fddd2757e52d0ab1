"""The job forms of the row-streaming kernels run a COPY of the single kernels' statements (csrc/linear_fwd_body.inc,
mlp_bwd_p1_body.inc: the single kernels keep their own text so that their code stays what it was).  The copies must be the kernels'
statements with only the workgroup coordinates respelled -- and, for the backward pass, the LDS declarations left to the caller and the last
workgroup counted among the job's workgroups.  No GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crfconv_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _kernel_statements(text, head, end):
    """The statements between the `) {` that closes the parameter list starting at `head` and the kernel's closing brace in front of `end`."""
    a = text.index(head)
    a = text.index(') {\n', a) + 4
    body = text[a:text.index(end, a)].rstrip()
    assert body.endswith('}')
    return body[:-1]


def _copy_statements(text):
    """An included file without its leading comment lines."""
    lines = text.split('\n')
    while lines and lines[0].startswith('//'):
        lines.pop(0)
    return '\n'.join(lines)


def test_linear_fwd_body_is_the_kernels_statements():
    src = _kernel_statements(_read('linear_fwd.hpp'), '__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_kernel(', '// The same statements as a device function')
    for a, b in (('blockIdx.x', 'LF_BX'), ('blockIdx.y', 'LF_BY'), ('gridDim.x', 'LF_NBX')):
        src = src.replace(a, b)
    assert not re.search(r'blockIdx|gridDim', src)
    assert src == _copy_statements(_read('linear_fwd_body.inc'))


def test_mlp_bwd_p1_body_is_the_kernels_statements():
    src = _kernel_statements(_read('mlp_bwd.hip'), '__global__ __launch_bounds__(WG_BLOCK) void mlp_bwd_p1_kernel(', '// The same statements as a device function')
    for drop in ('    __shared__ __attribute__((aligned(16))) float s_red[WG_WAVES][TCO * TCI * 256];\n',
                 '    __shared__ float s_v[WG_WAVES][(2 * TCO + TCI) * 16];\n',
                 '    __shared__ double s_own[ALIAS ? 1 : 5 * WG_BLOCK];\n', '    __shared__ int s_flag;\n'):
        assert src.count(drop) == 1
        src = src.replace(drop, '')
    last = 'last_workgroup(ticket, gridDim.x * gridDim.y * gridDim.z, &s_flag)'
    assert src.count(last) == 1
    src = src.replace(last, 'last_workgroup_of(ticket, P1_NBX * nby * nbz, &s_flag, P1_BX + P1_NBX * (P1_BY + nby * P1_BZ))')
    for a, b in (('blockIdx.x', 'P1_BX'), ('blockIdx.y', 'P1_BY'), ('blockIdx.z', 'P1_BZ'), ('gridDim.x', 'P1_NBX')):
        src = src.replace(a, b)
    assert not re.search(r'blockIdx|gridDim|__shared__', src)
    assert src == _copy_statements(_read('mlp_bwd_p1_body.inc'))


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
