"""Instruction and register counts of the four head_fwd_kernel variants from the compiler (no GPU needed); profiles/r13_eval_capture.md
quotes them.

    python scratch/head_isa_counts.py [--src crfconv_amd/csrc/head.hip] [--other OTHER/head.hip]

Compiles the file with the library's flags (csrc/Makefile) to gfx950 assembly and prints, per variant <NCH, EVAL>: MFMA
instructions, v_mul_lo_u32 (the dropout hash's multiplies, besides index arithmetic), global loads and stores, VGPRs, scratch bytes,
occupancy.  --other: a second source file (e.g. the parent commit's, whose kernel has no EVAL parameter); the instruction sequence of
its head_fwd_kernel<NCH> is compared with this file's <NCH, false> -- mnemonics and operands, labels left out."""
import argparse
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '-Wno-pass-failed', '--cuda-device-only', '-S']


def kernels(src):
    """{demangled-ish key: (instructions [str], metadata text)} of the head_fwd_kernel instantiations in `src`."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'head.s')
        subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + [src, '-o', out], cwd=os.path.dirname(src),
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = {}
    for m in re.finditer(r'^(_ZN3crf15head_fwd_kernelILi(\d)E(?:Lb([01])E)?EEv\w+):[^\n]*\n(.*?)^; Occupancy: (\d+)', text, re.S | re.M):
        body = m.group(4)
        code = body.split('.section', 1)[0] if '.rodata' in body else body
        ins = [re.sub(r'\s+', ' ', re.sub(r';.*', '', l)).strip() for l in code.splitlines()]
        ins = [i for i in ins if i and not i.startswith('.') and not i.endswith(':')]
        found[int(m.group(2)), m.group(3)] = (ins, body + '; Occupancy: ' + m.group(5))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--src', default=os.path.join(HERE, 'crfconv_amd', 'csrc', 'head.hip'))
    ap.add_argument('--other', default=None)
    a = ap.parse_args()
    mine = kernels(os.path.abspath(a.src))
    print('| head_fwd_kernel | MFMA | v_mul_lo_u32 | global loads | global stores | VGPRs | scratch | occupancy |')
    print('|---|---|---|---|---|---|---|---|')
    for (nch, ev), (ins, meta) in sorted(mine.items(), key=lambda kv: (kv[0][0], kv[0][1] or '')):
        count = lambda pat: sum(1 for i in ins if re.match(pat, i))           # noqa: E731
        field = lambda name: re.search(r'; %s: (\d+)' % name, meta).group(1)   # noqa: E731
        print('| <%d, %s> | %d | %d | %d | %d | %s | %s | %s |' % (nch, {'1': 'EVAL', '0': 'training', None: '-'}[ev], count('v_mfma'),
              count('v_mul_lo_u32'), count('global_load'), count('global_store'), field('NumVgprs'), field('ScratchSize'), field('Occupancy')))
    if a.other:
        theirs = kernels(os.path.abspath(a.other))
        strip = lambda ins: [re.sub(r'\.LBB\d+_\d+', 'L', i) for i in ins]      # noqa: E731
        for nch in (1, 2):
            old = theirs.get((nch, None)) or theirs.get((nch, '0'))
            same = strip(old[0]) == strip(mine[nch, '0'][0])
            print('head_fwd_kernel<%d> of %s against <%d, training> here: %d and %d instructions, sequences %s'
                  % (nch, a.other, nch, len(old[0]), len(mine[nch, '0'][0]), 'IDENTICAL' if same else 'DIFFER'))


if __name__ == '__main__':
    main()
