"""What drawing the random dilation in the finishing launch (graph.table_from_search_dilated, csrc/graph_table.hip) buys the sparse
networks that use dilated kNN graphs, and that the headline path kept its speed.  profiles/r22_dilated_tables.md holds what this prints.

    python scratch/dilated_tables_timing.py --what all --parent DIR [--out FILE.md]     # DIR: a checkout of the parent commit, built there
    python scratch/dilated_tables_timing.py --what finish|graph|step|bench [--tree DIR] [--mode parent|draw] [--net NAME]   # one leg, one JSON line

(a) finish   the finishing launch alone on the search table of 16 clouds x 8192 points (131 072 rows), (K, k) = (32, 16) and (64, 16):
             50 back-to-back calls between two device events, five times; beside it crfconv_graph_table at K = 16 on the same tree.
(b) graph    build_graph(as_table=True, method='knn', k=16, dilation=2 and 4) at 16 x 8192: with a DilationDraw (--mode draw, this tree)
             and without (--mode parent: knn_dilated + table_from_edges, the only path the parent has).
(c) step     CRFSegNet_Part / DualCRFSegNet (--net) forward + backward at 16 x 8192, graph_tables = True, with (--mode draw) and without
             (--mode parent) use_device_dilation.
(d) bench    `bench.py --gpus 1 --steps 100 --warmup 10` (ms per step, final_loss), on both trees.
`all` starts the legs as fresh processes, the two sides alternating, twice each.  (b), (c): host clock around the call plus a device
synchronise, median (and minimum) over TIMED calls after WARM."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from graph_tables_timing import sparse_batch, stats, wall      # noqa: E402  (the same batch and the same clock as r20)


def events(launch, calls=50, times=5):
    import torch
    for _ in range(10):
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
    return out


def leg_finish(dev, args):
    import torch
    from crfconv_amd import _lib
    from crfconv_amd.graph import stream_ptr
    from crfconv_amd.models import graph_ops
    pos, _, _, batch = sparse_batch(dev)
    n = pos.shape[0]
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    res = {}
    for K, k in ((32, 16), (64, 16)):
        nbr = graph_ops._knn_table(pos, pos, K, batch, batch)
        out = torch.empty((n, k), dtype=torch.int32, device=dev)
        us = events(lambda: _lib.call('crfconv_graph_table_dilated', nbr.data_ptr(), n, K, n, k, 5, counter.data_ptr(), 0, 0, out.data_ptr(),
                                      k, counts.data_ptr(), stream_ptr()))
        res['dilated_%d_%d' % (K, k)] = {'us_per_call': us, 'bytes': int(nbr.numel() * 4 + out.numel() * 4)}
    nbr = graph_ops._knn_table(pos, pos, 16, batch, batch)
    out = torch.empty((n, 16), dtype=torch.int32, device=dev)
    us = events(lambda: _lib.call('crfconv_graph_table', nbr.data_ptr(), n, 16, n, None, None, -1.0, 0, out.data_ptr(), 16,
                                  counts.data_ptr(), stream_ptr()))
    res['graph_table_16'] = {'us_per_call': us, 'bytes': int(nbr.numel() * 4 + out.numel() * 4)}
    return res


def leg_graph(dev, args):
    from crfconv_amd.models import point_conv as pc
    pos, _, _, batch = sparse_batch(dev)
    res = {}
    for d in (2, 4):
        how = {}
        if args.mode == 'draw':
            from crfconv_amd.models import graph_ops
            how['draw'] = graph_ops.DilationDraw(1, dev)
        tab = pc.build_graph(pos, batch, method='knn', k=16, dilation=d, as_table=True, **how)
        (ms,) = wall([lambda: pc.build_graph(pos, batch, method='knn', k=16, dilation=d, as_table=True, **how)])
        res['dilation_%d' % d] = dict(stats(ms), width=int(tab.K), n_edges=int(tab.n_edges))
    return res


def leg_step(dev, args):
    import torch
    import crfconv_amd
    from crfconv_amd import models
    from crfconv_amd.models import point_conv as pc
    pos, x, y, batch = sparse_batch(dev)
    data = crfconv_amd.Data(pos=pos, x=x, norm=x[:, 3:], batch=batch, category=torch.arange(16, device=dev) % 16)
    torch.manual_seed(3)
    net = getattr(models, args.net)(6, 13, steps=1).to(dev).train()
    net = pc.use_device_dilation(net, seed=3) if args.mode == 'draw' else pc.use_graph_tables(net)
    last = {}

    def step():
        torch.manual_seed(11)                                # the same torch.randint picks in every step of the parent's path
        net.zero_grad(set_to_none=True)
        out = net(data)
        last['loss'] = sum(torch.nn.functional.nll_loss(o, y) for o in (out if isinstance(out, tuple) else (out,)))
        last['loss'].backward()
    (ms,) = wall([step], warm=3, timed=20)
    return {'step': stats(ms), 'loss': float(last['loss'].detach())}


LEGS = {'finish': leg_finish, 'graph': leg_graph, 'step': leg_step}


def run_leg(what, tree, mode='draw', net='CRFSegNet_Part'):
    if what == 'bench':                                      # the benchmark itself, in the tree's own directory
        cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '100', '--warmup', '10']
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, cwd=os.path.abspath(tree) if tree else HERE)
    else:
        cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--mode', mode, '--net', net] + (['--tree', tree] if tree else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all', 'bench'] + sorted(LEGS))
    ap.add_argument('--tree', default=None, help='import crfconv_amd and benchlib from this checkout (built there)')
    ap.add_argument('--mode', default='draw', choices=['parent', 'draw'], help="draw: the device draw; parent: the parent's path")
    ap.add_argument('--net', default='CRFSegNet_Part', choices=['CRFSegNet_Part', 'DualCRFSegNet'])
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
    lines = ['command: python scratch/dilated_tables_timing.py --what all --parent <parent checkout>; ms, median (minimum)', '']

    def cell(d):
        return '%.3f (%.3f)' % (d['median_ms'], d['min_ms'])

    def flush():
        text = '\n'.join(lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return text
    f = run_leg('finish', None)
    lines.append('(a) the finishing launch alone, 131 072 rows, us per call over 50 calls, five times; bytes read + written; fraction of 8 TB/s at the median')
    for key in ('dilated_32_16', 'dilated_64_16', 'graph_table_16'):
        us = sorted(f[key]['us_per_call'])
        lines.append('    %-15s %s   %d bytes   %.3f' % (key, ' '.join('%.2f' % v for v in f[key]['us_per_call']), f[key]['bytes'],
                                                       f[key]['bytes'] / (us[2] * 1e-6) / 8e12))
    lines.append('')
    flush()
    order = (('parent', args.parent, 'parent'), ('this tree, no draw', None, 'parent'), ('this tree, draw', None, 'draw')) * 2
    runs = [(name, run_leg('graph', tree, mode)) for name, tree, mode in order]
    lines.append('(b) build_graph(as_table=True, k=16, dilation=d), 16 x 8192; fresh processes in this order: %s' % ', '.join(n for n, _ in runs))
    for d in (2, 4):
        for name in ('parent', 'this tree, no draw', 'this tree, draw'):
            rs = [r['dilation_%d' % d] for n, r in runs if n == name]
            lines.append('    d = %d  %-20s %s   width %d, %d edges' % (d, name, '   '.join(cell(r) for r in rs), rs[0]['width'], rs[0]['n_edges']))
    lines.append('')
    flush()
    for net in ('CRFSegNet_Part', 'DualCRFSegNet'):
        runs = [(mode, run_leg('step', None, mode, net)) for mode in ('parent', 'draw') * 2]
        lines.append('(c) %s(6, 13, steps=1) forward + backward, 16 x 8192, graph_tables = True; fresh processes in this order: %s'
                     % (net, ' '.join(m for m, _ in runs)))
        for mode, label in (('parent', 'knn_dilated'), ('draw', 'use_device_dilation')):
            lines.append('    %-20s %s   loss %s' % (label, '   '.join(cell(r['step']) for m, r in runs if m == mode),
                                                     ' '.join(repr(r['loss']) for m, r in runs if m == mode)))
        lines.append('')
        flush()
    runs = [(name, run_leg('bench', tree)) for name, tree in (('parent', args.parent), ('new', None)) * 2]
    lines.append('(d) fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'new'):
        lines.append('    bench.py ms_per_step %-6s %s   final_loss %s' % (name, ' '.join('%.4f' % r['ms_per_step'] for n, r in runs if n == name),
                                                                        ' '.join(repr(r['final_loss']) for n, r in runs if n == name)))
    lines.append('    final_loss equal in all four runs: %s' % (len({r['final_loss'] for _, r in runs}) == 1))
    lines.append('')
    print(flush())


if __name__ == '__main__':
    main()
