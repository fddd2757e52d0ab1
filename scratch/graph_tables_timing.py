"""What neighbour tables straight from the search (graph.table_from_search, csrc/graph_table.hip) buy the sparse path, and that the
headline path, whose narrowing now goes through the batched entry, kept its speed.  profiles/r20_graph_tables.md holds what this prints.

    python scratch/graph_tables_timing.py --what all --parent DIR [--out FILE.md]       # DIR: a checkout of the parent commit, built there
    python scratch/graph_tables_timing.py --what graph|step|headline|bench [--tree DIR] [--mode default|tables]      # one leg, one JSON line

(1) graph     one graph of 16 clouds x 8192 points, k = 16, from the positions to the table a symmetric PointConv layer consumes:
              knn_graph(loop=True) + the layer's self-loop handling + table_from_edges (the parent's path, restated here on
              ops.state.no_graph_tables) against knn_graph_table + the self-last finishing launch; same process, alternating call by
              call; the tables are compared with torch.equal.  The finishing launch alone: 50 back-to-back crfconv_graph_table calls
              between two device events.
(2) step      CRFSegNet(6, 13, steps=10) forward + backward at 16 x 8192: the parent's tree (--tree), this tree as it is (edge lists that
              carry their tables) and this tree with graph_tables = True.
(3) headline  CollateGraph.run at the benchmark shape with a checksum of its level-0 table, and `bench.py --gpus 1 --steps 100
              --warmup 10` (ms per step, final_loss), on both trees.
`all` starts the legs as fresh processes, parent and this tree alternating, twice each, so the spread of a tree against itself is seen
beside the difference between the trees.  Every timed figure: host clock around the call plus a device synchronise, median (and minimum)
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


def leg_graph(dev, mode):
    import torch
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import self_last_table, stream_ptr, table_from_edges
    from crfconv_amd.models import graph_ops
    pos, _, _, batch = sparse_batch(dev)
    n, k = pos.shape[0], 16

    def edge_path():                                         # the parent: search, edge list, the layer's loops, grouping by target
        ops.state.no_graph_tables = True
        try:
            ei = graph_ops.knn_graph(pos, k, batch, loop=True)
        finally:
            ops.state.no_graph_tables = False
        loops = torch.arange(n, dtype=ei.dtype, device=dev)
        ei = torch.cat([ei[:, ei[0] != ei[1]], torch.stack([loops, loops])], dim=1)
        return table_from_edges(ei[1], ei[0], n, n)

    def table_path():
        return self_last_table(graph_ops.knn_graph_table(pos, k, batch, loop=True))
    a, b = edge_path(), table_path()
    same = bool(torch.equal(a.idx32, b.idx32)) and a.n_edges == b.n_edges
    edge_ms, table_ms = wall([edge_path, table_path])
    # the finishing launch alone (the self-last form of the searched table), between two device events
    nbr = graph_ops.knn_graph_table(pos, k, batch, loop=True).idx32
    out = torch.empty((n, nbr.shape[1] + 1), dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def launch():
        _lib.call('crfconv_graph_table', nbr.data_ptr(), n, nbr.shape[1], n, None, None, -1.0, 2, out.data_ptr(), out.shape[1],
                  counts.data_ptr(), stream_ptr())
    for _ in range(10):
        launch()
    per_call = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / 50 * 1e3)
    return {'edge_path': stats(edge_ms), 'table_path': stats(table_ms), 'tables_equal': same, 'table_width': int(b.K),
            'n_edges': int(b.n_edges), 'finish_us_per_call': [float(v) for v in per_call],
            'finish_bytes': int(nbr.numel() * 4 + out.numel() * 4)}


def leg_step(dev, mode):
    import torch
    import crfconv_amd
    from crfconv_amd import models
    pos, x, y, batch = sparse_batch(dev)
    data = crfconv_amd.Data(pos=pos, x=x, batch=batch)
    torch.manual_seed(3)
    net = models.CRFSegNet(6, 13, steps=10).to(dev).train()
    if mode == 'tables':
        from crfconv_amd.models.point_conv import use_graph_tables
        use_graph_tables(net)
    last = {}

    def step():
        net.zero_grad(set_to_none=True)
        last['loss'] = torch.nn.functional.nll_loss(net(data), y)
        last['loss'].backward()
    (ms,) = wall([step], warm=3, timed=20)
    return {'step': stats(ms), 'loss': float(last['loss'])}


def leg_headline(dev, mode):
    import torch
    from benchlib.common import make_batch, synth_cloud
    from crfconv_amd.data import CollateGraph
    B, N = 4, 40960
    data, _ = make_batch(0, B, N, dev, torch.Generator().manual_seed(4242))
    clouds = [synth_cloud(9000 + i, N) for i in range(B)]
    pos = torch.from_numpy(np.stack([c[0] for c in clouds])).to(dev)
    x = torch.cat([pos, torch.from_numpy(np.stack([c[1] for c in clouds])).to(dev)], -1)
    y = torch.from_numpy(np.stack([c[2] for c in clouds])).to(dev)
    cg = CollateGraph(data, generator=torch.Generator().manual_seed(7))
    (cg_ms,) = wall([lambda: cg.run(pos, x, y)], warm=5, timed=50)
    level0 = zlib.crc32(data.multiscale[0].neighbor_idx.cpu().numpy().tobytes())
    return {'collate_graph_run': stats(cg_ms), 'collate_level0_crc32': level0}


LEGS = {'graph': leg_graph, 'step': leg_step, 'headline': leg_headline}


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
    lines = ['command: python scratch/graph_tables_timing.py --what all --parent <parent checkout>; WARM %d, TIMED %d; ms, median (minimum)'
             % (WARM, TIMED), '']

    def cell(d):
        return '%.3f (%.3f)' % (d['median_ms'], d['min_ms'])

    def flush():
        text = '\n'.join(lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return text
    g = run_leg('graph', None)
    lines += ['(1) one graph, 16 x 8192, k = 16, positions -> the self-last table of a symmetric PointConv layer; one process, alternating:',
              '    knn_graph + self-loop handling + table_from_edges   %s' % cell(g['edge_path']),
              '    knn_graph_table + self_loops=last                   %s' % cell(g['table_path']),
              '    tables equal: %s; width %d, %d edges' % (g['tables_equal'], g['table_width'], g['n_edges']),
              '    finishing launch alone, us per call over 50 calls, five times: %s  (%d bytes read + written)'
              % (' '.join('%.2f' % v for v in g['finish_us_per_call']), g['finish_bytes']), '']
    flush()
    order = (('parent', args.parent, 'default'), ('default', None, 'default'), ('tables', None, 'tables')) * 2
    runs = [(name, run_leg('step', tree, mode)) for name, tree, mode in order]
    lines.append('(2) CRFSegNet(6, 13, steps=10) forward + backward, 16 x 8192; fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'default', 'tables'):
        lines.append('    step %-8s %s   loss %s' % (name, '   '.join(cell(r['step']) for n, r in runs if n == name),
                                                   ' '.join(repr(r['loss']) for n, r in runs if n == name)))
    lines.append('')
    flush()
    runs = [(name, run_leg('headline', tree)) for name, tree in (('parent', args.parent), ('new', None)) * 2]
    lines.append('(3) fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'new'):
        lines.append('    collate_graph_run  %-6s %s' % (name, '   '.join(cell(r['collate_graph_run']) for n, r in runs if n == name)))
    lines.append('    collate_level0_crc32 equal in all four runs: %s' % (len({r['collate_level0_crc32'] for _, r in runs}) == 1))
    flush()
    runs = [(name, run_leg('bench', tree)) for name, tree in (('parent', args.parent), ('new', None)) * 2]
    for name in ('parent', 'new'):
        lines.append('    bench.py ms_per_step %-6s %s   final_loss %s' % (name, ' '.join('%.4f' % r['ms_per_step'] for n, r in runs if n == name),
                                                                        ' '.join(repr(r['final_loss']) for n, r in runs if n == name)))
    lines.append('    final_loss equal in all four runs: %s' % (len({r['final_loss'] for _, r in runs}) == 1))
    lines.append('')
    print(flush())


if __name__ == '__main__':
    main()
