"""What the register-resident farthest point sampling (csrc/fps.hip) costs and buys, against the parent commit's kernel (one form, the
running distances in global memory).  profiles/r21_fps.md holds what this prints.

    python scratch/fps_timing.py --what all --parent DIR [--out FILE.md]       # DIR: a checkout of the parent commit, built there
    python scratch/fps_timing.py --what fps|step|collate|headline|bench [--tree DIR] [--mode default|tables]      # one leg, one JSON line

(1) fps       graph_ops.fps(pos, batch, ratio=0.25) at 16 clouds x 8192, 2048, 512 and 128 points (the levels of the sparse pyramid), host
              clock; and the kernel alone, 20 back-to-back crfconv_fps calls between two device events, five times, as microseconds per
              call and per pick (a cloud's picks are strictly serial and the 16 clouds run side by side, so a call's time over the picks of
              ONE cloud is the time of one pick).  Also one cloud of 16 384, and 4 x 40 960 with 10 240 picks (the collate's shape).
(2) step      CRFSegNet(6, 13, steps=10) forward + backward at 16 x 8192, as it is and with graph_tables = True, with the loss.
(3) collate   multiscale_compute(sample_method='fps') at 4 x 40 960, with a checksum of every level's picks.
(4) headline  CollateGraph.run at the benchmark shape and `bench.py --gpus 1 --steps 100 --warmup 10` (no fps in either).
`all` starts the legs as fresh processes, parent and this tree alternating, twice each, so the spread of a tree against itself is seen
beside the difference between the trees.  The legs' own code is the same for both trees: the C entry and the Python calls they use exist
in both."""
import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_tables_timing as G      # wall, stats, sparse_batch and the step / headline legs are r20's  # noqa: E402


def crc(t):
    return zlib.crc32(t.cpu().numpy().tobytes())


def kernel_alone(pos, B, n, m, calls=20, times=5):
    """us per crfconv_fps call on B clouds of n points, m picks each, first pick row 0: `calls` back-to-back between two events."""
    import torch
    from crfconv_amd import _lib
    from crfconv_amd.graph import ptr, stream_ptr
    dev = pos.device
    ar = torch.arange(B, dtype=torch.int64, device=dev)
    starts, cnt = ar * n, torch.full((B,), n, dtype=torch.int64, device=dev)
    ostart, npick, first = ar * m, torch.full((B,), m, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    out, ws = torch.empty(B * m, dtype=torch.int64, device=dev), torch.empty(B * n, dtype=torch.float32, device=dev)
    p = pos.reshape(B * n, 3).contiguous()

    def launch():
        _lib.call('crfconv_fps', ptr(p), B, ptr(starts), ptr(cnt), ptr(ostart), ptr(npick), ptr(first), ptr(ws), ptr(out), stream_ptr())
    for _ in range(3):
        launch()
    per_call = []
    for _ in range(times):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            launch()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / calls * 1e3)
    return {'us_per_call': [float(v) for v in per_call], 'us_per_pick': float(np.median(per_call)) / max(m - 1, 1), 'crc32': crc(out)}


def leg_fps(dev, mode):
    import torch
    from benchlib.common import synth_cloud
    from crfconv_amd.models import graph_ops
    out = {}
    for n in (8192, 2048, 512, 128):
        pos = torch.from_numpy(np.concatenate([synth_cloud(7000 + i, n)[0] for i in range(16)])).to(dev)
        batch = torch.arange(16, device=dev).repeat_interleave(n)
        (ms,) = G.wall([lambda: graph_ops.fps(pos, batch, ratio=0.25)])
        out['16x%d' % n] = dict(G.stats(ms), picks_crc32=crc(graph_ops.fps(pos, batch, ratio=0.25)), kernel=kernel_alone(pos, 16, n, n // 4))
    pos = torch.from_numpy(synth_cloud(7100, 16384)[0]).to(dev)
    out['1x16384'] = {'kernel': kernel_alone(pos, 1, 16384, 4096, calls=5)}
    pos = torch.from_numpy(np.concatenate([synth_cloud(9000 + i, 40960)[0] for i in range(4)])).to(dev)
    out['4x40960'] = {'kernel': kernel_alone(pos, 4, 40960, 10240, calls=2)}
    return out


def leg_collate(dev, mode):
    import torch
    import crfconv_amd
    from benchlib.common import synth_cloud
    pos = torch.from_numpy(np.stack([synth_cloud(9000 + i, 40960)[0] for i in range(4)])).to(dev)
    last = {}

    def run():
        last['data'] = crfconv_amd.multiscale_compute(pos, sample_method='fps')
    (ms,) = G.wall([run], warm=2, timed=8)
    return {'multiscale_compute_fps': G.stats(ms), 'levels_crc32': [crc(lvl.pos) for lvl in last['data'].multiscale]}


LEGS = {'fps': leg_fps, 'step': G.leg_step, 'collate': leg_collate, 'headline': G.leg_headline}


def run_leg(what, tree, mode='default'):
    if what == 'bench':                                      # the benchmark itself, in the tree's own directory
        cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '100', '--warmup', '10']
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, cwd=os.path.abspath(tree) if tree else HERE)
    else:
        cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--mode', mode] + (['--tree', tree] if tree else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all', 'bench'] + sorted(LEGS))
    ap.add_argument('--tree', default=None, help='import crfconv_amd and benchlib from this checkout (built there)')
    ap.add_argument('--mode', default='default', choices=['default', 'tables'], help='step: graph_tables = True on every sparse layer')
    ap.add_argument('--parent', default=None, help='--what all: the checkout of the parent commit')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.what == 'bench':
        print(json.dumps(run_leg('bench', args.tree)))
        return
    if args.what != 'all':
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
        import torch
        assert torch.cuda.is_available(), 'a timing needs the GPU'
        print(json.dumps(LEGS[args.what]('cuda:0', args.mode)))
        return
    if not args.parent:
        raise SystemExit('--what all needs --parent DIR')
    lines = ['command: python scratch/fps_timing.py --what all --parent <parent checkout>; ms, median (minimum); fresh processes, parent and new alternating', '']

    def cell(d):
        return '%.3f (%.3f)' % (d['median_ms'], d['min_ms'])

    def flush():
        text = '\n'.join(lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return text
    pairs = (('parent', args.parent), ('new', None)) * 2
    runs = [(name, run_leg('fps', tree)) for name, tree in pairs]
    lines.append('(1) graph_ops.fps(pos, batch, 0.25), ms; kernel alone: us per call, five times | us per pick')
    for shape in ('16x8192', '16x2048', '16x512', '16x128', '1x16384', '4x40960'):
        for name in ('parent', 'new'):
            mine = [r[shape] for n, r in runs if n == name]
            lines.append('    %-8s %-6s %s   kernel %s' % (shape, name, '   '.join(cell(r) for r in mine if 'median_ms' in r),
                                                         '   '.join('%s | %.3f' % (' '.join('%.1f' % v for v in r['kernel']['us_per_call']), r['kernel']['us_per_pick'])
                                                                    for r in mine)))
        lines.append('    %-8s picks equal in all runs: %s' % (shape, len({(r[shape].get('picks_crc32'), r[shape]['kernel']['crc32']) for _, r in runs}) == 1))
    lines.append('')
    flush()
    order = (('parent', args.parent, 'default'), ('default', None, 'default'), ('parent-tables', args.parent, 'tables'), ('tables', None, 'tables')) * 2
    runs = [(name, run_leg('step', tree, mode)) for name, tree, mode in order]
    lines.append('(2) CRFSegNet(6, 13, steps=10) forward + backward, 16 x 8192; fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'default', 'parent-tables', 'tables'):
        lines.append('    step %-14s %s   loss %s' % (name, '   '.join(cell(r['step']) for n, r in runs if n == name),
                                                      ' '.join(repr(r['loss']) for n, r in runs if n == name)))
    lines.append('')
    flush()
    runs = [(name, run_leg('collate', tree)) for name, tree in pairs]
    lines.append('(3) multiscale_compute(sample_method=fps), 4 x 40 960')
    for name in ('parent', 'new'):
        lines.append('    %-6s %s' % (name, '   '.join(cell(r['multiscale_compute_fps']) for n, r in runs if n == name)))
    lines.append('    every level equal in all four runs: %s' % (len({tuple(r['levels_crc32']) for _, r in runs}) == 1))
    lines.append('')
    flush()
    runs = [(name, run_leg('headline', tree)) for name, tree in pairs]
    lines.append('(4) fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'new'):
        lines.append('    collate_graph_run  %-6s %s' % (name, '   '.join(cell(r['collate_graph_run']) for n, r in runs if n == name)))
    lines.append('    collate_level0_crc32 equal in all four runs: %s' % (len({r['collate_level0_crc32'] for _, r in runs}) == 1))
    flush()
    runs = [(name, run_leg('bench', tree)) for name, tree in pairs]
    for name in ('parent', 'new'):
        lines.append('    bench.py ms_per_step %-6s %s   final_loss %s' % (name, ' '.join('%.4f' % r['ms_per_step'] for n, r in runs if n == name),
                                                                        ' '.join(repr(r['final_loss']) for n, r in runs if n == name)))
    lines.append('    final_loss equal in all four runs: %s' % (len({r['final_loss'] for _, r in runs}) == 1))
    lines.append('')
    print(flush())


if __name__ == '__main__':
    main()
