"""Per-kernel comparison of the gfx950 device code of two trees (no GPU needed); profiles/r14_pointconv_split.md and r16_crf_split.md quote it.

    python scratch/kernel_code_diff.py --left A.hip [B.hip ...] --right C.hip [D.hip ...]
    python scratch/kernel_code_diff.py --left OLD/csrc/build --right crfconv_amd/csrc/build

A side is a set of source files, compiled here with the library's flags (csrc/Makefile) plus --cuda-device-only, or a build directory,
whose *.o have their gfx950 code object unbundled.  Per kernel symbol of either side: only-left, only-right, identical or DIFFERS, with
the number of instruction encoding words up to the kernel's last s_endpgm, and the resource block of the code object's metadata (SGPRs,
VGPRs, AGPRs, scratch, LDS, spills; from source also the occupancy of the compiler's resource-usage remarks).  The two sides are only
compared with each other.  Exit status 1 when a kernel that both sides have differs.  --rename REGEX REPL matches the kernels by their
demangled names after that substitution: a kernel whose parameter list changed (profiles/r15_gemm_split.md)."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '-Wno-pass-failed', '--cuda-device-only',
         '--no-gpu-bundle-output', '-Rpass-analysis=kernel-resource-usage']
FIELDS = ['sgpr_count', 'vgpr_count', 'agpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'sgpr_spill_count',
          'vgpr_spill_count']


def code_object(path, tmp):
    """(code object file, {kernel: occupancy}) of a source file or a host object."""
    out = os.path.join(tmp, '%d.co' % len(os.listdir(tmp)))
    if not path.endswith('.o'):
        p = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + ['-c', path, '-o', out], cwd=os.path.dirname(path),
                           stderr=subprocess.PIPE, text=True)
        if p.returncode:
            sys.exit(p.stderr)
        occ = dict(re.findall(r'remark: Function Name: (\S+) .*?Occupancy \[waves/SIMD\]: (\d+)', p.stderr, re.S))
        return out, occ
    fat = out + '.fatbin'
    if subprocess.call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, path], stderr=subprocess.DEVNULL):
        return None, {}                                                        # a unit without device code
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fat, '--output=' + out,
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950'])
    return out, {}


def kernels_of(co, occ):
    """{kernel symbol: (encoding words up to the last s_endpgm, resource tuple)}."""
    if co is None:
        return {}
    notes = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    res = {}
    for block in re.split(r'^  - \.agpr_count:', notes, flags=re.M)[1:]:
        block = '.agpr_count:' + block
        name = re.search(r'^\s+\.name:\s+(\S+)', block, re.M).group(1)
        res[name] = tuple(int(re.search(r'\.%s:\s+(\d+)' % f, block).group(1)) for f in FIELDS) + (occ.get(name, '-'),)
    found, cur = {}, None
    for line in subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', co], text=True).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = m.group(1) if m.group(1) in res else None
            if cur:
                found[cur] = [[], 0]
            continue
        m = cur and re.search(r'//\s*[0-9A-F]+:((?:\s[0-9A-F]{8})+)', line)
        if m:
            words, _ = found[cur]
            words += m.group(1).split()
            if line.split()[0] == 's_endpgm':
                found[cur][1] = len(words)
    return {k: (tuple(w[:n]), res[k]) for k, (w, n) in found.items()}


def side(paths, tmp):
    files = []
    for p in paths:
        files += sorted(glob.glob(os.path.join(p, '*.o'))) if os.path.isdir(p) else [os.path.abspath(p)]
    per_unit = [(os.path.basename(f), kernels_of(*code_object(f, tmp))) for f in files]
    units_of = {}
    for unit, ks in per_unit:
        for k in ks:
            units_of.setdefault(k, []).append(unit)
    # a kernel of a shared header is compiled in every unit that launches it: such a symbol is compared unit by unit
    return {k if len(units_of[k]) == 1 else '%s @%s' % (k, os.path.splitext(unit)[0]): v + (unit,) for unit, ks in per_unit for k, v in ks.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--left', nargs='+', required=True)
    ap.add_argument('--right', nargs='+', required=True)
    ap.add_argument('-q', '--quiet', action='store_true', help='list only the kernels that are not identical')
    ap.add_argument('--rename', nargs=2, metavar=('REGEX', 'REPL'),
                    help='re.sub on the demangled names of both sides before matching (a kernel whose parameter list changed)')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        left, right = side(a.left, tmp), side(a.right, tmp)
    names = sorted(set(left) | set(right))
    filt = shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('c++filt')             # (mangled names without one)
    base = [k.split(' @')[0] for k in names]
    plain = subprocess.check_output([filt] + base, text=True).splitlines() if filt and names else base
    pretty = {k: p + k[len(b):] for k, b, p in zip(names, base, plain)}
    if a.rename:                                             # kernels are matched by their demangled, rewritten names
        pretty = {k: re.sub(a.rename[0], a.rename[1], p) for k, p in pretty.items()}
        left, right = ({pretty[k]: v for k, v in s.items()} for s in (left, right))
        names = sorted(set(left) | set(right))
        pretty = {k: k for k in names}
    count = {'only-left': 0, 'only-right': 0, 'identical': 0, 'DIFFERS': 0}
    words = 0
    for k in names:
        lw, rw = left.get(k), right.get(k)
        if lw is None or rw is None:
            what = 'only-left' if rw is None else 'only-right'
            detail = '%d words, %s' % (len((lw or rw)[0]), (lw or rw)[2])
        else:
            same_code, same_res = lw[0] == rw[0], lw[1] == rw[1]
            what = 'identical' if same_code and same_res else 'DIFFERS'
            detail = '%d / %d words, %s / %s' % (len(lw[0]), len(rw[0]), lw[2], rw[2])
            if not same_res:
                detail += ', resources %s / %s' % (lw[1], rw[1])
            words += len(lw[0]) if what == 'identical' else 0
        count[what] += 1
        if not (a.quiet and what == 'identical'):
            print('%-10s %s  (%s)' % (what, pretty[k], detail))
    print('left %d kernels, right %d; only-left %d, only-right %d, identical %d (%d words, resources %s), differing %d'
          % (len(left), len(right), count['only-left'], count['only-right'], count['identical'], words,
             ' '.join(FIELDS + ['occupancy']), count['DIFFERS']))
    return 1 if count['DIFFERS'] else 0


if __name__ == '__main__':
    sys.exit(main())
