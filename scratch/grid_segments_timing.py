"""What the grid subsampling of a ragged batch on the device (crfconv_amd/grid.py, csrc/grid_subsample.hip) costs, against the only route the
tree had before it: the batch to the host, ``utils.cpp_subsampling.compute`` per cloud, the results back to the device -- and what the
host entry ``compute`` itself costs, before and after it moved onto the shared kernels.  profiles/r35_grid_segments.md holds what this prints.

    python scratch/grid_segments_timing.py --what op|route|compute --shape batch|single|host [--tree DIR]      # one leg, one JSON line
    python scratch/grid_segments_timing.py --what all --parent DIR [--out FILE.md]       # every leg as a fresh process, new and parent alternating

Shapes:  batch   16 clouds x 262 144 points in about 8 x 6 x 3 m, size 0.164        (about 8 points per voxel)
         single  one cloud of 2^22 points in about 60 x 45 x 8 m, size 0.345
         host    one cloud of 2^20 points in about 30 x 30 x 8 m, size 0.19: the shape of the `compute` leg
All with F = 3 features and L = 1 label column.
Legs:    op       grid.grid_subsample, the whole call with its one host read: device events around back-to-back calls
         route    pos / x / y .cpu(), compute() per cloud, torch.cat and back to the device: host clock around the whole route, synchronised
         compute  cpp_subsampling.compute on host arrays: host clock
--tree DIR imports crfconv_amd from DIR (the parent commit exported and built there) instead of this tree."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {'batch': dict(clouds=16, n=1 << 18, box=(8.0, 6.0, 3.0), size=0.164),
          'single': dict(clouds=1, n=1 << 22, box=(60.0, 45.0, 8.0), size=0.345),
          'host': dict(clouds=1, n=1 << 20, box=(30.0, 30.0, 8.0), size=0.19)}


def make(shape):
    sh = SHAPES[shape]
    rng = np.random.default_rng(3500)
    parts = [(rng.random((sh['n'], 3)) * np.asarray(sh['box']) + 10.0 * s).astype(np.float32) for s in range(sh['clouds'])]
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    pos = np.concatenate(parts)
    x = rng.uniform(0.0, 255.0, (len(pos), 3)).astype(np.float32)
    y = rng.integers(0, 13, (len(pos), 1)).astype(np.int32)
    return pos, ptr, x, y


def event_ms(fn, calls, times=5, warm=2):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(times):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return [float(v) for v in out]


def host_ms(fn, times=5, warm=1, sync=False):
    import torch
    out = []
    for k in range(warm + times):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out


def leg_op(shape):
    import torch
    from crfconv_amd import grid
    pos_h, ptr_h, x_h, y_h = make(shape)
    size = SHAPES[shape]['size']
    pos, ptr, x, y = (torch.from_numpy(a).cuda() for a in (pos_h, ptr_h, x_h, y_h))
    got = grid.grid_subsample(pos, ptr, size=size, x=x, y=y)
    N, M = len(pos_h), got.pos.shape[0]
    # the reduction's algorithmic bytes: the sorted ids, the voxels' starts, every input row gathered once, every output row written
    return {'M': M, 'N': N, 'whole_ms': event_ms(lambda: grid.grid_subsample(pos, ptr, size=size, x=x, y=y), 10),
            'reduce_bytes': 4 * N + 8 * M + N * (12 + 12 + 4) + M * (12 + 12 + 4 + 4)}


def leg_route(shape):
    import torch
    from crfconv_amd.utils import cpp_subsampling
    pos_h, ptr_h, x_h, y_h = make(shape)
    size = SHAPES[shape]['size']
    pos, x, y = (torch.from_numpy(a).cuda() for a in (pos_h, x_h, y_h))
    last = {}

    def route():
        p, f, c = pos.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy()
        outs = [cpp_subsampling.compute(p[a:b], features=f[a:b], classes=c[a:b], sampleDl=size) for a, b in zip(ptr_h[:-1], ptr_h[1:])]
        last['out'] = [torch.from_numpy(np.concatenate([o[k] for o in outs])).cuda() for k in range(3)]
    ms = host_ms(route, times=3, sync=True)
    return {'M': int(last['out'][0].shape[0]), 'N': len(pos_h), 'whole_ms': ms}


def leg_compute(shape):
    from crfconv_amd.utils import cpp_subsampling
    pos_h, _, x_h, y_h = make(shape)
    size = SHAPES[shape]['size']
    last = {}

    def call():
        last['out'] = cpp_subsampling.compute(pos_h, features=x_h, classes=y_h, sampleDl=size)
    ms = host_ms(call, times=7, warm=2)
    import zlib
    return {'M': int(last['out'][0].shape[0]), 'N': len(pos_h), 'whole_ms': ms,
            'crc': [zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in last['out']]}


LEGS = {'op': leg_op, 'route': leg_route, 'compute': leg_compute}


def run_leg(what, shape, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--shape', shape] + (['--tree', tree] if tree else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def fmt(runs):
    return '   '.join('%.3f (%.3f)' % (np.median(r['whole_ms']), min(r['whole_ms'])) for r in runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all'] + sorted(LEGS))
    ap.add_argument('--shape', default='batch', choices=sorted(SHAPES))
    ap.add_argument('--tree', default=None)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
    if args.what != 'all':
        print(json.dumps(LEGS[args.what](args.shape)))
        return
    if not args.parent:
        raise SystemExit('--what all needs --parent DIR: the parent commit, exported and built')
    lines = ['command: python scratch/grid_segments_timing.py --what all --parent DIR; ms per call, median (minimum); fresh processes', '']

    def flush():
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    for shape in ('batch', 'single'):
        ops, routes = [], []
        for _ in range(5):                                  # new and parent alternating
            ops.append(run_leg('op', shape))
            routes.append(run_leg('route', shape, args.parent))
        sh = SHAPES[shape]
        lines.append('%s: %d cloud(s) x %d points, size %g, M = %d voxels (route: %d)' % (shape, sh['clouds'], sh['n'], sh['size'], ops[0]['M'], routes[0]['M']))
        lines.append('    grid.grid_subsample          %s' % fmt(ops))
        lines.append('    parent route (host compute)  %s' % fmt(routes))
        lines.append('    reduction algorithmic bytes  %.1f MB' % (ops[0]['reduce_bytes'] / 1e6))
        lines.append('')
        flush()
    new, old = [], []
    for _ in range(5):
        new.append(run_leg('compute', 'host'))
        old.append(run_leg('compute', 'host', args.parent))
    med = lambda rs: [float(np.median(r['whole_ms'])) for r in rs]                      # noqa: E731
    lo, hi = min(med(old)), max(med(old))
    lines.append('cpp_subsampling.compute, one cloud of 2^20 points, M = %d (parent %d); outputs equal (crc): %s'
                 % (new[0]['M'], old[0]['M'], len({tuple(r['crc']) for r in new + old}) == 1))
    lines.append('    new     %s' % fmt(new))
    lines.append('    parent  %s' % fmt(old))
    lines.append('    parent range of medians %.3f .. %.3f, widened by its spread: %.3f .. %.3f; new medians inside: %s'
                 % (lo, hi, lo - (hi - lo), hi + (hi - lo), all(lo - (hi - lo) <= v <= hi + (hi - lo) for v in med(new))))
    flush()
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
