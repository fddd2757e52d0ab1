"""What one segmented kNN search per graph buys the sparse path, and that the uniform entry (the headline collate) kept its speed.
profiles/r18_knn_segments.md holds what this prints.

    python scratch/knn_segments_timing.py --what all --parent DIR [--out FILE.md]      # DIR: a checkout of the parent commit, built there
    python scratch/knn_segments_timing.py --what graph|step|headline [--tree DIR]      # one leg, one JSON line (what `all` starts)

(1) graph     graph_ops.knn_graph(pos, 16, batch, loop=True) at 16 clouds x 8192 points (the ScanNet / NPM3D configuration) against the
              per-cloud loop over knn_batch_device it replaces, restated here; same process, alternating call by call; the edge lists
              are compared with array_equal.
(2) step      CRFSegNet(6, 13, steps=10) forward + backward at 16 x 8192, on this tree and on the parent's (--tree).
(3) headline  knn_batch_device at 4 x 40960, K = 16 self-queries, and CollateGraph.run at the benchmark shape, on both trees; a checksum
              of the neighbour table on the same seeded input is printed by both and compared by `all`.
`all` starts the legs as fresh processes, parent and this tree alternating, twice each, so the spread of a tree against itself is seen
beside the difference between the trees.  Every figure: host clock around the call plus a device synchronise, median (and minimum)
over TIMED calls after WARM."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TIMED = 5, 25


def wall(fns, warm=WARM, timed=TIMED):
    """ms [timed] per function of `fns`, the functions taking turns call by call; each call ends with a device synchronise."""
    import torch
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(timed):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) * 1e3)
    return out


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms))}


def sparse_batch(dev, B=16, N=8192):
    import torch
    from benchlib.common import synth_cloud
    clouds = [synth_cloud(7000 + i, N) for i in range(B)]
    pos = torch.from_numpy(np.concatenate([c[0] for c in clouds])).to(dev)
    x = torch.cat([pos, torch.from_numpy(np.concatenate([c[1] for c in clouds])).to(dev)], -1)
    y = torch.from_numpy(np.concatenate([c[2] for c in clouds])).to(dev) - 1
    batch = torch.arange(B, device=dev).repeat_interleave(N)
    return pos, x, y, batch


def leg_graph(dev):
    import torch
    from crfconv_amd.models import graph_ops
    from crfconv_amd.utils import nearest_neighbors as nn_
    pos, _, _, batch = sparse_batch(dev)
    k = 16

    def per_cloud_loop():                                    # what knn_graph(loop=True) was: one search per cloud, host read included
        counts = torch.bincount(batch).tolist()
        rows, cols, o = [], [], 0
        for c in counts:
            kk = min(k, c)
            idx = nn_.knn_batch_device(pos[o:o + c].unsqueeze(0), pos[o:o + c].unsqueeze(0), kk)[0]
            rows.append(torch.arange(o, o + c, device=dev).unsqueeze(1).expand(-1, kk).reshape(-1))
            cols.append((idx + o).reshape(-1))
            o += c
        return torch.stack([torch.cat(cols), torch.cat(rows)])

    def segmented():
        return graph_ops.knn_graph(pos, k, batch, loop=True)
    same = bool(torch.equal(per_cloud_loop(), segmented()))
    loop_ms, seg_ms = wall([per_cloud_loop, segmented])
    return {'per_cloud_loop': stats(loop_ms), 'segmented': stats(seg_ms), 'edge_lists_equal': same}


def leg_step(dev):
    import torch
    import crfconv_amd
    from crfconv_amd import models
    pos, x, y, batch = sparse_batch(dev)
    data = crfconv_amd.Data(pos=pos, x=x, batch=batch)
    torch.manual_seed(3)
    net = models.CRFSegNet(6, 13, steps=10).to(dev).train()

    def step():
        net.zero_grad(set_to_none=True)
        torch.nn.functional.nll_loss(net(data), y).backward()
    (ms,) = wall([step], warm=3, timed=20)
    return {'step': stats(ms)}


def leg_headline(dev):
    import torch
    from benchlib.common import make_batch, synth_cloud
    from crfconv_amd.data import CollateGraph
    from crfconv_amd.utils import nearest_neighbors as nn_
    B, N, K = 4, 40960, 16
    data, _ = make_batch(0, B, N, dev, torch.Generator().manual_seed(4242))
    clouds = [synth_cloud(9000 + i, N) for i in range(B)]
    pos = torch.from_numpy(np.stack([c[0] for c in clouds])).to(dev)
    x = torch.cat([pos, torch.from_numpy(np.stack([c[1] for c in clouds])).to(dev)], -1)
    y = torch.from_numpy(np.stack([c[2] for c in clouds])).to(dev)
    table = nn_.knn_batch_device(pos, pos, K)
    check = zlib.crc32(table.cpu().numpy().tobytes())
    (knn_ms,) = wall([lambda: nn_.knn_batch_device(pos, pos, K)], warm=10, timed=100)
    cg = CollateGraph(data, generator=torch.Generator().manual_seed(7))
    (cg_ms,) = wall([lambda: cg.run(pos, x, y)], warm=5, timed=50)
    level0 = zlib.crc32(data.multiscale[0].neighbor_idx.cpu().numpy().tobytes())
    return {'knn_batch_device': stats(knn_ms), 'collate_graph_run': stats(cg_ms), 'knn_table_crc32': check, 'collate_level0_crc32': level0}


LEGS = {'graph': leg_graph, 'step': leg_step, 'headline': leg_headline}


def run_leg(what, tree):
    cmd = [sys.executable, os.path.abspath(__file__), '--what', what] + (['--tree', tree] if tree else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all'] + sorted(LEGS))
    ap.add_argument('--tree', default=None, help='import crfconv_amd and benchlib from this checkout (built there)')
    ap.add_argument('--parent', default=None, help='--what all: the checkout of the parent commit')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.what != 'all':
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
        import torch
        assert torch.cuda.is_available(), 'a timing needs the GPU'
        print(json.dumps(LEGS[args.what]('cuda:0')))
        return
    if not args.parent:
        raise SystemExit('--what all needs --parent DIR')
    lines = ['command: python scratch/knn_segments_timing.py --what all --parent <parent checkout>; WARM %d, TIMED %d; ms, median (minimum)' % (WARM, TIMED), '']

    def cell(d):
        return '%.3f (%.3f)' % (d['median_ms'], d['min_ms'])
    g = run_leg('graph', None)
    lines += ['(1) knn_graph(pos, 16, batch, loop=True), 16 x 8192, one process, alternating:',
              '    per-cloud loop over knn_batch_device  %s' % cell(g['per_cloud_loop']),
              '    one segmented search                  %s' % cell(g['segmented']),
              '    edge lists equal: %s' % g['edge_lists_equal'], '']
    for what, keys in (('step', ['step']), ('headline', ['knn_batch_device', 'collate_graph_run'])):
        runs = [(name, run_leg(what, tree)) for name, tree in (('parent', args.parent), ('new', None)) * 2]
        lines.append('(%s) fresh processes in this order: %s' % ('2' if what == 'step' else '3', ' '.join(n for n, _ in runs)))
        for key in keys:
            for name in ('parent', 'new'):
                lines.append('    %-18s %-6s %s' % (key, name, '   '.join(cell(r[key]) for n, r in runs if n == name)))
        if what == 'headline':
            for key in ('knn_table_crc32', 'collate_level0_crc32'):
                lines.append('    %s equal in all four runs: %s' % (key, len({r[key] for _, r in runs}) == 1))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
