"""What the ragged-batch transforms (transforms.SegmentCompose: crfconv_augment_segments and crfconv_fixed_points, csrc/augment_segments.hip)
cost beside the per-cloud framework composition a user of the parent writes, and that the headline path kept its speed.
profiles/r24_segment_transforms.md holds what this prints.

    python scratch/segment_transforms_timing.py --what all --parent DIR [--out FILE.md]     # DIR: a checkout of the parent commit, built there
    python scratch/segment_transforms_timing.py --what launch|headline|bench [--tree DIR]  # one leg, one JSON line

(a) launch    the augment launch (NormalizeScale, rotate, anisotropic scale, one flip axis, noise, normals, x = [pos, norm]) and the picks
              launch (FixedPoints(2048), the three modes) on 16 x 8192 points, on 16 clouds of uneven sizes summing to 131 072 and on one
              cloud of 65 536: 50 back-to-back calls between two device events, five times after 10 calls.  Beside them the same chain
              written cloud by cloud with framework operators (the same given parameters; its noise is torch.randn), timed the same way
              with 5 calls per window.  Algorithmic bytes: pos and norm read once, pos, norm and x [N, 6] written once (72 N); the
              picks: 8 bytes per pick written.
(b) headline  CollateGraph.run at the benchmark shape (graph_tables_timing.leg_headline) and `bench.py --gpus 1 --steps 100 --warmup 10`,
              fresh processes, parent and new alternating, twice each."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from graph_tables_timing import leg_headline      # noqa: E402  (the same headline leg as r20 .. r23)

UNEVEN = [1, 37, 512, 1000, 2048, 3000, 4096, 4097, 6000, 8192, 9000, 12000, 16384, 20000, 24000]      # + the rest: 16 clouds, 131 072 rows


def events(launch, calls=50, times=5, warm=10):
    import torch
    for _ in range(warm):
        launch()
    out = []
    for _ in range(times):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            launch()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return [float(v) for v in out]


def framework_chain(pos, norm, ptr_host, params, sigma=0.01, clip=0.05):
    """The chain cloud by cloud with framework operators, as a user of the parent writes it: NormalizeScale, RandomRotate about z,
    RandomScaleAnisotropic, RandomSymmetry on x, RandomNoise, the normals carried along, x = [pos, norm]."""
    import torch
    out_p, out_n = [], []
    for b in range(len(ptr_host) - 1):
        p, n = pos[ptr_host[b]:ptr_host[b + 1]], norm[ptr_host[b]:ptr_host[b + 1]]
        p = p - p.mean(0)
        p = p * ((1 / p.abs().max()) * 0.999999)
        c, s = params[b, 0], params[b, 1]
        zero, one = torch.zeros_like(c), torch.ones_like(c)
        M = torch.stack([torch.stack([c, s, zero]), torch.stack([-s, c, zero]), torch.stack([zero, zero, one])])
        p, n = (p @ M) * params[b, 2:5], (n @ M) / params[b, 2:5]
        n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-30)
        p = torch.cat([(p[:, :1].max() - p[:, :1]), p[:, 1:]], 1)
        n = n * torch.tensor([-1.0, 1.0, 1.0], device=n.device)
        p = p + (sigma * torch.randn_like(p)).clamp(-clip, clip)
        out_p.append(p), out_n.append(n)
    p, n = torch.cat(out_p), torch.cat(out_n)
    return p, n, torch.cat([p, n], 1)


def leg_launch(dev, args):
    import torch
    from crfconv_amd import transforms as T
    rng = np.random.default_rng(0)
    shapes = {'16 x 8192': [8192] * 16, '16 uneven': UNEVEN + [131072 - sum(UNEVEN)], '1 x 65536': [65536]}
    res = {}
    for name, sizes in shapes.items():
        S, N = len(sizes), sum(sizes)
        ptr_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pos0 = torch.from_numpy((rng.uniform(-1, 1, (N, 3)) * [3, 2, 1] + 200).astype(np.float32)).to(dev)
        nrm = rng.standard_normal((N, 3))
        norm0 = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        ptr = torch.from_numpy(ptr_host).to(dev)
        chain = T.SegmentCompose([T.NormalizeScale(), T.RandomRotate(180, axis=2), T.RandomScaleAnisotropic([0.8, 1.2]),
                                  T.RandomSymmetry([True, False, False]), T.RandomNoise(0.01), T.AddFeatsByKeys([True, True], ['pos', 'norm'])],
                                 generator=torch.Generator().manual_seed(1))
        host = chain.draws(chain.seed, 0, S)['params']
        host[:, 5] = 1                                       # every cloud flips: the composition does the same work for all
        params = torch.from_numpy(host).to(dev)
        pos, norm, x = pos0.clone(), norm0.clone(), torch.empty((N, 6), device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        # (in place, call after call: the cloud is normalised again each time; the work per call does not depend on the values)
        aug = events(lambda: chain.apply_segments(pos, norm, x, ptr, chain.seed, counter, params_in=params))
        fw = events(lambda: framework_chain(pos0, norm0, ptr_host, params), calls=5, warm=2)
        row = {'S': S, 'N': N, 'augment_us': aug, 'augment_bytes': 72 * N, 'framework_us': fw}
        for mode, fixed in (('replace', T.FixedPoints(2048)), ('subset', T.FixedPoints(2048, replace=False)),
                            ('duplicates', T.FixedPoints(2048, replace=False, allow_duplicates=True))):
            pick = T.SegmentCompose([fixed], generator=torch.Generator().manual_seed(2))
            out_host = np.concatenate([[0], np.cumsum(fixed.counts(sizes))]).astype(np.int64)
            out_ptr, M = torch.from_numpy(out_host).to(dev), int(out_host[-1])
            row['picks_%s_us' % mode] = events(lambda: pick.pick(ptr, out_ptr, N, M, pick.seed, counter))
            row['picks_%s_bytes' % mode] = 8 * M
        # what the parent's user writes for FixedPoints(2048, replace=True): one randint and one index per cloud
        row['picks_framework_us'] = events(lambda: torch.cat([int(ptr_host[b]) + torch.randint(0, int(sizes[b]), (2048,), device=dev)
                                                              for b in range(S)]), calls=5, warm=2)
        res[name] = row
    return res


LEGS = {'launch': leg_launch, 'headline': lambda dev, args: leg_headline(dev, 'default')}


def run_leg(what, tree):
    import subprocess
    if what == 'bench':                                      # the benchmark itself, in the tree's own directory
        cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '100', '--warmup', '10']
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, cwd=os.path.abspath(tree) if tree else HERE)
    else:
        cmd = [sys.executable, os.path.abspath(__file__), '--what', what] + (['--tree', tree] if tree else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all', 'bench'] + sorted(LEGS))
    ap.add_argument('--tree', default=None, help='import crfconv_amd and benchlib from this checkout (built there)')
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
        print(json.dumps(LEGS[args.what]('cuda:0', args)))
        return
    if not args.parent:
        raise SystemExit('--what all needs --parent DIR')
    lines = ['command: python scratch/segment_transforms_timing.py --what all --parent <parent checkout>', '']

    def flush():
        text = '\n'.join(lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return text

    def us(v):
        return ' '.join('%.2f' % u for u in v)
    launch = run_leg('launch', None)
    lines.append('(a) us per call, five windows; bytes; fraction of 8 TB/s at the median window')
    for name, r in launch.items():
        lines.append('    %s (S = %d, N = %d)' % (name, r['S'], r['N']))
        lines.append('        augment launch        %s   %d bytes   %.4f' % (us(r['augment_us']), r['augment_bytes'],
                                                                         r['augment_bytes'] / (sorted(r['augment_us'])[2] * 1e-6) / 8e12))
        lines.append('        framework, per cloud  %s' % us(r['framework_us']))
        for mode in ('replace', 'subset', 'duplicates'):
            v, nb = r['picks_%s_us' % mode], r['picks_%s_bytes' % mode]
            lines.append('        picks, %-14s %s   %d bytes   %.4f' % (mode, us(v), nb, nb / (sorted(v)[2] * 1e-6) / 8e12))
        lines.append('        picks, framework      %s' % us(r['picks_framework_us']))
    lines.append('')
    flush()
    runs = []
    for name, tree in (('parent', args.parent), ('new', None)) * 2:
        runs.append((name, run_leg('headline', tree), run_leg('bench', tree)))
    lines.append('(b) fresh processes in this order: %s' % ' '.join(n for n, _, _ in runs))
    for name in ('parent', 'new'):
        mine = [(h, b) for n, h, b in runs if n == name]
        lines.append('    CollateGraph.run ms, median (minimum) %-6s %s   level-0 crc32 %s'
                     % (name, '   '.join('%.3f (%.3f)' % (h['collate_graph_run']['median_ms'], h['collate_graph_run']['min_ms']) for h, _ in mine),
                        ' '.join(str(h['collate_level0_crc32']) for h, _ in mine)))
        lines.append('    bench.py ms_per_step %-6s %s   final_loss %s' % (name, ' '.join('%.4f' % b['ms_per_step'] for _, b in mine),
                                                                        ' '.join(repr(b['final_loss']) for _, b in mine)))
    lines.append('    final_loss equal in all four runs: %s' % (len({b['final_loss'] for _, _, b in runs}) == 1))
    lines.append('')
    print(flush())


if __name__ == '__main__':
    main()
