"""What the part IoU of a ragged batch on the device (utils.PartScores, csrc/part_scores.hip) costs against the two routes the tree had before
it: the per-shape loop around ``runningScoreShapeNet.update`` and a batched composition of framework kernels.
profiles/r36_part_scores.md holds what this prints.

    python scratch/part_scores_timing.py --what op|route|torch --shape s16|s64       # one leg, one JSON line
    python scratch/part_scores_timing.py --what all [--out FILE.md]                  # every leg as a fresh process, alternating, five runs each

Shapes:  s16  16 shapes x 2048 rows, C = 50;  s64  64 shapes x 2048 rows, C = 50.  Categories cycle through the 16 of ShapeNet.
Legs:    op     PartScores.update(y, ptr, category, scores=out): device events around back-to-back calls, and the same call captured in a
                graph of 20 updates (the device's own time, without the host's launch cost)
         route  the parent's route: per shape, a slice, a framework arg-max and runningScoreShapeNet.update (two host reads each): host clock
                around the whole batch, synchronised
         torch  a batched framework composition: the category's columns masked, arg-max, one bincount over (shape, truth, prediction), the
                ratios in float64 on the device and one host read of the [S] values: device events around back-to-back calls
All legs run on this tree; the routes use nothing this change adds."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {'s16': 16, 's64': 64}
ROWS, C, HBM = 2048, 50, 8.0e12


def make(shape):
    import torch
    from crfconv_amd.utils import PartScores
    S = SHAPES[shape]
    rng = np.random.default_rng(3600)
    ps = PartScores.shapenet('cuda')
    category = np.arange(S) % 16
    y = np.concatenate([rng.choice(ps.parts[c], ROWS) for c in category]).astype(np.int64)
    scores = rng.standard_normal((S * ROWS, C)).astype(np.float32)
    scores[np.arange(len(y)), y] += 2.0
    ptr = (np.arange(S + 1) * ROWS).astype(np.int64)
    return ps, [torch.from_numpy(a).cuda() for a in (y, scores, ptr, category.astype(np.int64))], category


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


def leg_op(shape):
    import torch
    ps, (y, scores, ptr, category), _ = make(shape)
    eager = event_ms(lambda: ps.update(y, ptr, category, scores=scores), 50)
    with_pred = event_ms(lambda: ps.update(y, ptr, category, scores=scores, return_preds=True), 50)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ps.update(y, ptr, category, scores=scores)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(20):
            ps.update(y, ptr, category, scores=scores)
    captured = [v / 20 for v in event_ms(graph.replay, 5)]
    N = y.numel()
    return {'whole_ms': eager, 'with_pred_ms': with_pred, 'graph_ms': captured, 'bytes': N * (4 * C + 8), 'pred_bytes': 8 * N,
            'iou0': float(ps.update(y, ptr, category, scores=scores)[0])}


def leg_route(shape):
    import torch
    from crfconv_amd.utils import runningScoreShapeNet
    _, (y, scores, ptr, _), category = make(shape)
    bounds = ptr.tolist()
    out, last = [], {}
    for k in range(1 + 5):
        score = runningScoreShapeNet('cuda')
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s, c in enumerate(category):
            a, b = bounds[s], bounds[s + 1]
            last[s] = score.update(y[a:b], scores[a:b].max(dim=1)[1], int(c))
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t) * 1e3)
    return {'whole_ms': out, 'iou0': float(last[0])}


def leg_torch(shape):
    import torch
    ps, (y, scores, ptr, category), _ = make(shape)
    S = category.numel()
    member = torch.zeros((16, C), dtype=torch.bool, device='cuda')
    for c, lst in enumerate(ps.parts):
        member[c, lst] = True
    n_parts = member.sum(dim=1)
    eps = float(np.finfo(np.float32).eps)

    def call():
        shape_of = torch.repeat_interleave(torch.arange(S, device='cuda'), ptr[1:] - ptr[:-1])
        allowed = member[category][shape_of]
        pred = scores.masked_fill(~allowed, float('-inf')).argmax(dim=1)
        hist = torch.bincount((shape_of * C + y) * C + pred, minlength=S * C * C).view(S, C, C)
        inter = hist.diagonal(dim1=1, dim2=2).double()
        union = hist.sum(dim=2).double() + hist.sum(dim=1).double() - inter
        ratio = ((inter + eps) / (union + eps)) * member[category]
        return (ratio.sum(dim=1) / n_parts[category]).cpu()
    return {'whole_ms': event_ms(call, 20), 'iou0': float(call()[0])}


LEGS = {'op': leg_op, 'route': leg_route, 'torch': leg_torch}


def run_leg(what, shape):
    cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--shape', shape]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def fmt(runs, key='whole_ms'):
    return '   '.join('%.4f (%.4f)' % (np.median(r[key]), min(r[key])) for r in runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all'] + sorted(LEGS))
    ap.add_argument('--shape', default='s16', choices=sorted(SHAPES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.what != 'all':
        print(json.dumps(LEGS[args.what](args.shape)))
        return
    lines = ['command: python scratch/part_scores_timing.py --what all; ms per batch, median (minimum) of each of five fresh processes', '']
    for shape in ('s16', 's64'):
        runs = {k: [] for k in LEGS}
        for _ in range(5):                                  # the legs alternate
            for k in ('op', 'route', 'torch'):
                runs[k].append(run_leg(k, shape))
        op = runs['op']
        best = min(min(r['graph_ms']) for r in op) * 1e-3
        lines.append('%s: %d shapes x %d rows, C = %d; first shape IoU op / route / torch: %.6f / %.6f / %.6f'
                     % (shape, SHAPES[shape], ROWS, C, op[0]['iou0'], runs['route'][0]['iou0'], runs['torch'][0]['iou0']))
        lines.append('    PartScores.update, eager               %s' % fmt(op))
        lines.append('    PartScores.update, eager, with preds   %s' % fmt(op, 'with_pred_ms'))
        lines.append('    PartScores.update, in a captured graph %s' % fmt(op, 'graph_ms'))
        lines.append('    per-shape loop (parent route)          %s' % fmt(runs['route']))
        lines.append('    batched framework composition          %s' % fmt(runs['torch']))
        lines.append('    algorithmic bytes N (4 C + 8) = %.2f MB (+ %.2f MB with pred_out); fastest captured update %.2f us = %.2f TB/s = %.1f %% of 8 TB/s'
                     % (op[0]['bytes'] / 1e6, op[0]['pred_bytes'] / 1e6, best * 1e6, op[0]['bytes'] / best / 1e12, 100 * op[0]['bytes'] / best / HBM))
        lines.append('')
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
