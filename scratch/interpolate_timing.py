"""What the fused kNN interpolation (csrc/interp.hip, ops.interpolate) costs against the framework composition it replaced, and what it
does to a whole sparse step.  profiles/r19_interpolate.md holds what this prints.

    python scratch/interpolate_timing.py --what all --parent DIR [--out FILE.md]     # DIR: a checkout of the parent commit, built there
    python scratch/interpolate_timing.py --what interp|step [--tree DIR]             # one leg, one JSON line (what `all` starts)
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scratch/interpolate_timing.py --what kernels --channels 64
    python scratch/trace_avg.py DIR interp_                                          # the two launches' own times

(1) interp    models.knn_interpolate forward + backward, 16 x 8192 targets from their fps subsets at ratio 0.25 (16 x 2048 sources), k = 3,
              at C = 64 and C = 512, on this tree (one HIP launch each way) and on the parent's (--tree: gathers, two index_add_ and a
              divide, autograd's scatters behind them).  On this tree also: the forward launch alone (device events around 50 back-to-back
              calls over a prebuilt table) with its algorithmic bytes, the in-degrees of the table, and whether two runs give the same bits.
    kernels   the same shape at ONE width (--channels): 20 forward launches and 20 transposed ones, nothing timed here -- for a kernel trace.
(2) step      CRFSegNet(6, 13, steps=10) forward + backward at 16 x 8192, and how many parameter gradients differ in any bit between two
              such steps from the same state.
`all` starts the legs as fresh processes, parent and this tree alternating, twice each, so the spread of a tree against itself is seen
beside the difference between the trees.  Timed figures: host clock around the call plus a device synchronise, median (and minimum)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12


def wall(fn, warm, timed):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(timed):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': float(np.median(out)), 'min_ms': float(np.min(out))}


def sparse_batch(dev, B=16, N=8192):
    import torch
    from benchlib.common import synth_cloud
    clouds = [synth_cloud(7000 + i, N) for i in range(B)]
    pos = torch.from_numpy(np.concatenate([c[0] for c in clouds])).to(dev)
    x = torch.cat([pos, torch.from_numpy(np.concatenate([c[1] for c in clouds])).to(dev)], -1)
    y = torch.from_numpy(np.concatenate([c[2] for c in clouds])).to(dev) - 1
    batch = torch.arange(B, device=dev).repeat_interleave(N)
    return pos, x, y, batch


def leg_interp(dev):
    import torch
    from crfconv_amd import models, ops
    from crfconv_amd.models import graph_ops
    pos, _, _, batch = sparse_batch(dev)
    pick = graph_ops.fps(pos, batch, ratio=0.25)
    sub_pos, sub_batch = pos[pick], batch[pick]
    n_y, n_x, k = pos.shape[0], sub_pos.shape[0], 3
    out = {'n_y': n_y, 'n_x': n_x}
    col = graph_ops.knn(sub_pos, pos, k, sub_batch, batch)[1]
    deg = torch.bincount(col, minlength=n_x)
    out['in_degree'] = {'median': int(deg.median()), 'max': int(deg.max())}
    gen = torch.Generator(device=dev).manual_seed(5)
    for C in (64, 512):
        x = (torch.rand((n_x, C), device=dev, generator=gen) + 0.5).requires_grad_()
        g = torch.rand((n_y, C), device=dev, generator=gen) + 0.5

        def fwd_bwd():
            x.grad = None
            o = models.knn_interpolate(x, sub_pos, pos, sub_batch, batch, k)
            o.backward(g)
            return o
        res = {'fwd_bwd': wall(fwd_bwd, 5, 30)}
        a = fwd_bwd().detach().clone()
        ga = x.grad.clone()
        b = fwd_bwd().detach()
        res['same_bits_twice'] = bool(torch.equal(a, b) and torch.equal(ga, x.grad))
        if hasattr(ops, 'interpolate'):
            from crfconv_amd.graph import table_from_index
            from crfconv_amd.utils import nearest_neighbors as nn_
            ptr = lambda ids: torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(ids, minlength=16), 0)])
            table = table_from_index(nn_.knn_segments_device(sub_pos, ptr(sub_batch), pos, ptr(batch), k, out_dtype=torch.int32), n_x)
            xd = x.detach()
            for _ in range(5):
                ops.interpolate(xd, sub_pos, pos, table)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                ops.interpolate(xd, sub_pos, pos, table)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 50
            nbytes = n_y * (12 + 4 * k + 4 * C) + n_x * (12 + 4 * C)          # no coef written without a gradient: the 4 K term once
            res['forward_call'] = {'us': us, 'algorithmic_bytes': nbytes, 'fraction_of_8TBps': nbytes / (us * 1e-6) / PEAK_BYTES_PER_S}
        out['C%d' % C] = res
    return out


def leg_kernels(dev, C):
    import torch
    from crfconv_amd import ops
    from crfconv_amd.models import graph_ops
    pos, _, _, batch = sparse_batch(dev)
    pick = graph_ops.fps(pos, batch, ratio=0.25)
    sub_pos, sub_batch = pos[pick], batch[pick]
    x = (torch.rand((sub_pos.shape[0], C), device=dev) + 0.5).requires_grad_()
    g = torch.rand((pos.shape[0], C), device=dev) + 0.5
    for _ in range(20):
        x.grad = None
        ops.knn_interpolate(x, sub_pos, pos, sub_batch, batch, 3).backward(g)
    torch.cuda.synchronize()
    return {'channels': C, 'launches_each_way': 20}


def leg_step(dev):
    import torch
    import crfconv_amd
    from crfconv_amd import models
    pos, x, y, batch = sparse_batch(dev)
    data = crfconv_amd.Data(pos=pos, x=x, batch=batch)
    torch.manual_seed(3)
    net = models.CRFSegNet(6, 13, steps=10).to(dev).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def step():
        net.zero_grad(set_to_none=True)
        torch.nn.functional.nll_loss(net(data), y).backward()
    out = {'step': wall(step, 3, 20)}
    grads = []
    for _ in range(2):                                       # two steps from the same state (running statistics included)
        net.load_state_dict(state)
        step()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    differ = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    out['gradients'] = {'tensors': len(grads[0]), 'differ_in_some_bit': len(differ)}
    return out


LEGS = {'interp': leg_interp, 'step': leg_step, 'kernels': leg_kernels}


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
    ap.add_argument('--channels', type=int, default=64, help='--what kernels: the width')
    args = ap.parse_args()
    if args.what != 'all':
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
        import torch
        assert torch.cuda.is_available(), 'a timing needs the GPU'
        print(json.dumps(LEGS[args.what]('cuda:0', args.channels) if args.what == 'kernels' else LEGS[args.what]('cuda:0')))
        return
    if not args.parent:
        raise SystemExit('--what all needs --parent DIR')
    cell = lambda d: '%.3f (%.3f)' % (d['median_ms'], d['min_ms'])
    lines = ['command: python scratch/interpolate_timing.py --what all --parent <parent checkout>; ms, median (minimum)', '']
    order = (('parent', args.parent), ('new', None)) * 2
    runs = [(name, run_leg('interp', tree)) for name, tree in order]
    new = [r for n, r in runs if n == 'new'][0]
    lines += ['(1) models.knn_interpolate forward + backward, %d targets from %d sources, k = 3; fresh processes in this order: %s'
              % (new['n_y'], new['n_x'], ' '.join(n for n, _ in runs)),
              '    in-degree of the table: median %d, maximum %d' % (new['in_degree']['median'], new['in_degree']['max'])]
    for C in ('C64', 'C512'):
        for name in ('parent', 'new'):
            mine = [r[C] for n, r in runs if n == name]
            lines.append('    %-5s %-6s %s   same bits twice: %s' % (C, name, '   '.join(cell(r['fwd_bwd']) for r in mine),
                                                                    ' '.join(str(r['same_bits_twice']) for r in mine)))
        for r in (r[C] for n, r in runs if n == 'new'):
            f = r['forward_call']
            lines.append('    %-5s forward call alone: %.1f us, %d algorithmic bytes, %.3f of 8 TB/s' % (C, f['us'], f['algorithmic_bytes'], f['fraction_of_8TBps']))
    lines.append('')
    runs = [(name, run_leg('step', tree)) for name, tree in order]
    lines.append('(2) CRFSegNet(6, 13, steps=10) forward + backward, 16 x 8192; fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
    for name in ('parent', 'new'):
        mine = [r for n, r in runs if n == name]
        lines.append('    step %-6s %s   gradient tensors that differ between two steps from one state: %s'
                     % (name, '   '.join(cell(r['step']) for r in mine),
                        ' '.join('%d of %d' % (r['gradients']['differ_in_some_bit'], r['gradients']['tensors']) for r in mine)))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
