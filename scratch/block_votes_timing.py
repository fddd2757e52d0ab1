"""What the merge of per-block scores onto the points costs (crfconv_amd/blocks.py: BlockVotes, csrc/block_votes.hip), against the
framework composition a user writes today.  profiles/r34_block_votes.md holds what this prints.

    python scratch/block_votes_timing.py --what all [--out FILE.md]        # every leg as a fresh process, the two ways alternating, five times
    python scratch/block_votes_timing.py --what op|torch --shape npm3d|scannet        # one leg, one JSON line

Shapes (those of scratch/sliding_blocks_timing.py):
         npm3d    one scene of 2^20 points in about 60 x 45 x 8 m at the NPM3D parameters, C = 9
         scannet  16 scenes of 65 536 points in about 8 x 6 x 3 m at the ScanNet parameters, C = 20
Ways:    op       split.reverse() (the library call, on a fresh table every time), votes.update (core='prefer'; exp False and True),
                  votes.result('mean')
         torch    sums.index_add_(0, split.rows, scores) alone, and then bincount, the division and the arg-max
Device times are between two device events around `calls` back-to-back calls, after warm-up calls.
The update's algorithmic bytes: the scores read once (4 R C), the inverse table (8 (N + 1) + 4 R), sums read and written (8 N C)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'scratch'))

from sliding_blocks_timing import SHAPES, event_ms, make          # noqa: E402

CLASSES = {'npm3d': 9, 'scannet': 20}


def setup(shape):
    import torch
    from crfconv_amd import blocks
    pos_h, ptr_h = make(shape)
    prm = getattr(blocks, SHAPES[shape]['params'])
    split = blocks.sliding_blocks(torch.from_numpy(pos_h).cuda(), torch.from_numpy(ptr_h).cuda(), **prm)
    C = CLASSES[shape]
    gen = torch.Generator(device='cuda').manual_seed(3400)
    scores = torch.log_softmax(torch.randn((split.n_rows, C), device='cuda', generator=gen), 1)
    return split, scores, C, len(pos_h)


def leg_op(shape):
    import torch
    from crfconv_amd import _lib, blocks
    from crfconv_amd.graph import ptr as p_, stream_ptr
    split, scores, C, N = setup(shape)
    R = split.n_rows
    out = {'n_blocks': split.n_blocks, 'n_rows': R, 'C': C}
    nbytes = _lib.call('crfconv_block_reverse_workspace', N, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    rev_ptr, packed = torch.empty(N + 1, dtype=torch.int64, device='cuda'), torch.empty(R, dtype=torch.int32, device='cuda')
    out['reverse_ms'] = event_ms(lambda: _lib.call('crfconv_block_reverse', p_(split.rows), R, N, p_(split.mask), p_(ws), nbytes, p_(rev_ptr),
                                                   p_(packed), stream_ptr()), 20)
    assert torch.equal(rev_ptr, split.reverse()[0]) and torch.equal(packed & 0x7fffffff, split.reverse()[1])
    for exp in (False, True):
        votes = blocks.BlockVotes(split, C, exp=exp)
        out['update_exp_ms' if exp else 'update_ms'] = event_ms(lambda: votes.update(scores), 20)
    out['result_ms'] = event_ms(lambda: votes.result('mean'), 20)
    out['covered'] = int((votes.count > 0).sum())
    out['algorithmic_bytes'] = 4 * R * C + 8 * (N + 1) + 4 * R + 8 * N * C
    return out


def leg_torch(shape):
    import torch
    split, scores, C, N = setup(shape)
    sums = torch.zeros((N, C), dtype=torch.float32, device='cuda')
    out = {'n_blocks': split.n_blocks, 'n_rows': split.n_rows, 'C': C}
    out['index_add_ms'] = event_ms(lambda: sums.index_add_(0, split.rows, scores), 20)

    def rest():
        count = torch.bincount(split.rows, minlength=N)
        return sums / count.clamp(min=1)[:, None], sums.argmax(1)
    out['rest_ms'] = event_ms(rest, 20)
    a = torch.zeros_like(sums).index_add_(0, split.rows, scores)
    b = torch.zeros_like(sums).index_add_(0, split.rows, scores)
    out['two_runs_differ_in'] = int((a.view(torch.int32) != b.view(torch.int32)).sum())
    return out


LEGS = {'op': leg_op, 'torch': leg_torch}


def run_leg(what, shape):
    cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--shape', shape]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all'] + sorted(LEGS))
    ap.add_argument('--shape', default='npm3d', choices=sorted(SHAPES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.what != 'all':
        print(json.dumps(LEGS[args.what](args.shape)))
        return
    lines = ['command: python scratch/block_votes_timing.py --what all; ms per call, median (minimum) of five windows of 20 calls; fresh '
             'processes, the two ways alternating, five runs each', '']
    fmt = lambda runs, key: '   '.join('%.4f (%.4f)' % (np.median(r[key]), min(r[key])) for r in runs)          # noqa: E731
    for shape in ('npm3d', 'scannet'):
        runs = [(what, run_leg(what, shape)) for what in ('op', 'torch') * 5]
        op, fw = [r for w, r in runs if w == 'op'], [r for w, r in runs if w == 'torch']
        lines.append('%s: %d scene(s) x %d points, blocks %d rows %d C %d, covered points %d' % (
            shape, SHAPES[shape]['scenes'], SHAPES[shape]['n'], op[0]['n_blocks'], op[0]['n_rows'], op[0]['C'], op[0]['covered']))
        for key in ('reverse_ms', 'update_ms', 'update_exp_ms', 'result_ms'):
            lines.append('    op     %-14s %s' % (key, fmt(op, key)))
        for key in ('index_add_ms', 'rest_ms'):
            lines.append('    torch  %-14s %s' % (key, fmt(fw, key)))
        best_op, best_fw = min(min(r['update_ms']) for r in op), min(min(r['index_add_ms']) for r in fw)
        lines.append('    minimum of the five runs: update %.4f ms, index_add_ %.4f ms -> update is %s (ratio %.2f)' % (
            best_op, best_fw, 'not slower' if best_op <= best_fw else 'SLOWER', best_fw / best_op))
        lines.append('    update: %.1f MB algorithmic -> %.0f GB/s at the median of the first run (%.1f %% of 8 TB/s)' % (
            op[0]['algorithmic_bytes'] / 1e6, op[0]['algorithmic_bytes'] / np.median(op[0]['update_ms']) / 1e6,
            op[0]['algorithmic_bytes'] / np.median(op[0]['update_ms']) / 1e6 / 80.0))
        lines.append('    index_add_: words that differ between two runs on the same input: %s' % [r['two_runs_differ_in'] for r in fw])
        lines.append('')
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
