"""One captured replay of the optimizer step ALONE over the parameters of PointConvBig(6, 13) (820 141 float32 elements):
optim.FlatAdam without and with global-norm clipping, optim.FlatSGD, and torch.optim.Adam in the forms this torch offers on ROCm
(foreach, and fused=True if it constructs; both capturable=True, which a captured torch Adam needs).  profiles/r11_flat_adam.md holds
the table this prints.

    python scratch/flat_adam_timing.py [--replays 200] [--rounds 6] [--out FILE.md]

Every variant owns a copy of the model and one hipGraph of its step().  After a warm-up round the variants alternate within one
process for `rounds` rounds (their order rotates from round to round); a sample is `replays` replays between two device events, a
device synchronise behind them.  Reported: median and min - max of the per-replay time, launches per step, and the algorithmic bytes of
an Adam step (28 B per element: read p, g, m, v, write p, m, v; 32 B with amsgrad) over the median -- vectors of 3.3 MB stay in the
caches between replays, so that rate is NOT a share of HBM bandwidth.  The launch counts of the torch variants are taken last, from
one eager step under torch.profiler (the timing table is printed before)."""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from crfconv_amd import models, optim                                                   # noqa: E402
from crfconv_amd.distributed import FlatGradAllReduce                                   # noqa: E402


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('flat_adam_timing: needs the GPU (a CPU run gives no time)')
    dev = 'cuda'
    torch.manual_seed(0)
    base = models.PointConvBig(6, 13).to(dev)
    n = sum(p.numel() for p in base.parameters() if p.requires_grad)
    gen = torch.Generator(device=dev).manual_seed(1)
    arms, launches, notes, keep = {}, {}, {}, []

    def flat(name, make, nl):
        net = copy.deepcopy(base)
        bucket = FlatGradAllReduce(net)
        opt = make(bucket)
        bucket.flat.normal_(generator=gen).mul_(1e-2)
        keep.append((net, bucket, opt))
        arms[name], launches[name] = capture(opt.step), nl
    flat('FlatAdam', lambda b: optim.FlatAdam(b, lr=1e-3, weight_decay=1e-4, check_every=0), 2)
    flat('FlatAdam, max_grad_norm', lambda b: optim.FlatAdam(b, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, check_every=0), 3)
    flat('FlatSGD', lambda b: optim.FlatSGD(b, lr=1e-2, momentum=0.95, weight_decay=1e-4, check_every=0), 1)
    eager_steps = {}
    for name, kw in (('torch.optim.Adam foreach', dict(foreach=True)), ('torch.optim.Adam fused', dict(fused=True))):
        net = copy.deepcopy(base)
        params = [p for p in net.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.empty_like(p).normal_(generator=gen).mul_(1e-2)
        try:
            opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-4, capturable=True, **kw)
            arms[name] = capture(opt.step)
        except Exception as e:                               # this torch does not offer the form on this device
            notes[name] = 'not available: %s' % str(e).splitlines()[0][:120]
            continue
        keep.append((net, opt))
        eager_steps[name] = opt.step
        launches[name] = None
        notes[name] = '%d parameter tensors' % len(params)

    def timed(graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.replays          # us per replay

    names = list(arms)
    for nm in names:                                         # warm-up round at the timed length
        timed(arms[nm])
    us = {nm: [] for nm in names}
    for rnd in range(a.rounds):
        for i in range(len(names)):
            nm = names[(i + rnd) % len(names)]
            us[nm].append(timed(arms[nm]))

    def table():
        lines = ['| variant | launches per step | median us per replay | min | max | algorithmic GB/s (28 B x n / median) | note |',
                 '|---|---|---|---|---|---|---|']
        for nm in names:
            v = sorted(us[nm])
            med = v[len(v) // 2]
            rate = '%.0f' % (28.0 * n / med / 1e3) if 'Adam' in nm else '--'
            lines.append('| `%s` | %s | %.2f | %.2f | %.2f | %s | %s |' % (nm, 'not counted' if launches[nm] is None else launches[nm], med,
                                                                          v[0], v[-1], rate, notes.get(nm, '')))
        for nm, why in notes.items():
            if nm not in arms:
                lines.append('| `%s` | -- | -- | -- | -- | -- | %s |' % (nm, why))
        return ('n = %d elements, %d replays per sample, %d rounds after one warm-up round\n\n' % (n, a.replays, a.rounds)) + '\n'.join(lines)

    def emit():
        text = table()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(text + '\n')
        return text
    print(emit(), flush=True)
    # launches of the torch variants: device kernels of one eager step
    from torch.profiler import ProfilerActivity, profile
    for nm, step in eager_steps.items():
        try:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            launches[nm] = sum(1 for ev in prof.events() if str(getattr(ev, 'device_type', '')).endswith('CUDA'))
        except Exception as e:
            notes[nm] += '; launches not counted (%s)' % str(e).splitlines()[0][:80]
    print(emit(), flush=True)
    print(json.dumps({'n': n, 'replays': a.replays, 'rounds': a.rounds, 'us_per_replay': us, 'launches': launches, 'notes': notes}))


if __name__ == '__main__':
    main()
