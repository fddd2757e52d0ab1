"""The eval forward of PointConvBig with CRF decoders four ways, in one process: (a) model.eval() eager, (b) the same as one hipGraph,
(c) InferenceNet eager, (d) InferenceNet as one hipGraph.  profiles/r12_infer.md holds the tables this prints.

    python scratch/infer_timing.py [--calls 200] [--config c2|c5|all] [--out FILE.md]
    python scratch/infer_timing.py --trace b|d --config c2|c5        (under rocprofv3 --kernel-trace --stats: one variant alone)
    python scratch/infer_timing.py --stats FILE_kernel_stats.csv      (launches and summed kernel time per forward from that run)

Shapes: BASELINE config 2 (4 x 40 960 points, K 16, T 3, 13 classes) and the config-5 crop (1 x 65 536, K 32, T 5, 8 classes), the
synthetic clouds of bench.py.  Every variant is timed TWICE (`a#1`, `a#2`): the variants alternate call by call within a pass, each
call sits between two HIP events of its own, and the two passes run one after the other.  Reported per variant: the median of each
pass over `calls` calls after a warm-up, and the spread = |median#1 - median#2|.  (a) and (b) are the eval path as it is without
InferenceNet; a gain is claimed only where (d) < (b) or (c) < (a) by more than the larger of the two variants' spreads.  The eager
variants include the host's launch work (the stream runs dry between launches); the captured ones are device time.  The outputs of
(c) / (d) are checked to be torch.equal to (a) before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import crfconv_amd                                                                       # noqa: E402
from benchlib.common import synth_cloud                                                  # noqa: E402
from crfconv_amd import InferenceNet, models                                             # noqa: E402

CONFIGS = {'c2': ('BASELINE config 2: 4 x 40 960 points, K = 16, T = 3', 4, 40960, 16, 3, 13),
           'c5': ('config-5 crop: 1 x 65 536 points, K = 32, T = 5', 1, 65536, 32, 5, 8)}


def make(dev, B, N, K, T, C, seed):
    clouds = [synth_cloud(seed + i, N) for i in range(B)]
    pos = torch.from_numpy(np.stack([c[0] for c in clouds])).to(dev)
    x = torch.cat([pos, torch.from_numpy(np.stack([c[1] for c in clouds])).to(dev)], -1)
    data = crfconv_amd.multiscale_compute(pos, x=x, kernel_size=(K,) * 5, generator=torch.Generator().manual_seed(seed), sort='morton')
    torch.manual_seed(seed)
    net = models.PointConvBig(6, C, use_crf=True, steps=T).to(dev)
    with torch.no_grad():                                    # a used network's BatchNorm state, not a fresh module's mean 0 / variance 1
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return data, net.eval()


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = fn()
    return graph, out


def variants(dev, key):
    _, B, N, K, T, C = CONFIGS[key]
    data, net = make(dev, B, N, K, T, C, 500 + N % 89)
    fast = InferenceNet(net)
    with torch.no_grad():
        ref = net(data)
        assert torch.equal(fast(data), ref), 'InferenceNet differs from model.eval()'
    gb, ob = capture(lambda: net(data))
    gd, od = capture(lambda: fast(data))
    gb.replay()
    gd.replay()
    torch.cuda.synchronize()
    assert torch.equal(ob, ref) and torch.equal(od, ref), 'a captured forward differs from the eager one'

    def eager(model):
        def run():
            with torch.no_grad():
                model(data)
        return run
    return {'a': eager(net), 'b': gb.replay, 'c': eager(fast), 'd': gd.replay}, (net, fast, data, gb, gd, ob, od)


def time_config(dev, key, calls, warm):
    arms, keep = variants(dev, key)
    names = list(arms)
    med = {}
    for rep in (1, 2):
        for _ in range(warm):
            for nm in names:
                arms[nm]()
        torch.cuda.synchronize()
        evs = {nm: [] for nm in names}
        for i in range(calls):
            for j in range(len(names)):
                nm = names[(i + j) % len(names)]            # the order rotates from call to call
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                arms[nm]()
                e1.record()
                evs[nm].append((e0, e1))
            if i % 25 == 24:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        for nm in names:
            med[nm, rep] = float(np.median([a.elapsed_time(b) for a, b in evs[nm]]))
    del keep
    return med


TRACE_REPLAYS = 20
TRACE_FORWARDS = TRACE_REPLAYS + 3          # capture()'s three eager warm-up forwards run the same launches


WHAT = {'a': '`model.eval()` eager', 'b': '`model.eval()` captured', 'c': '`InferenceNet` eager', 'd': '`InferenceNet` captured'}


def table(key, med, calls):
    lines = ['### %s' % CONFIGS[key][0], '', '%d calls per variant and pass, HIP events around every call, variants alternating' % calls, '',
             '| variant | median ms, pass 1 | median ms, pass 2 | spread ms |', '|---|---|---|---|']
    spread = {}
    for nm in 'abcd':
        spread[nm] = abs(med[nm, 1] - med[nm, 2])
        lines.append('| (%s) %s | %.4f | %.4f | %.4f |' % (nm, WHAT[nm], med[nm, 1], med[nm, 2], spread[nm]))
    lines.append('')
    for new, old in (('d', 'b'), ('c', 'a')):
        m_new, m_old = 0.5 * (med[new, 1] + med[new, 2]), 0.5 * (med[old, 1] + med[old, 2])
        s = max(spread[new], spread[old])
        verdict = 'a gain beyond the spread' if m_old - m_new > s else ('a loss beyond the spread' if m_new - m_old > s else 'within the spread')
        lines.append('(%s) against (%s): %.4f ms against %.4f ms, difference %+.4f ms (%+.1f %%), spread %.4f ms: %s' %
                     (new, old, m_new, m_old, m_new - m_old, 100.0 * (m_new - m_old) / m_old, s, verdict))
        lines.append('')
    return '\n'.join(lines)


def stats_summary(path):
    """Launches and summed kernel time per forward from the kernel statistics of a --trace run: the kernels whose call count is a
    multiple of TRACE_FORWARDS are the forward's (the collate's and the set-up's are called a handful of times each)."""
    import csv
    rows = list(csv.DictReader(open(path)))
    fwd = [r for r in rows if int(r['Calls']) % TRACE_FORWARDS == 0]
    launches = sum(int(r['Calls']) for r in fwd) // TRACE_FORWARDS
    ns = sum(float(r['TotalDurationNs']) for r in fwd) / TRACE_FORWARDS
    other = sum(float(r['TotalDurationNs']) for r in rows) - ns * TRACE_FORWARDS
    lines = ['%d launches per forward, %.1f us summed kernel time per forward (%d kernel names; %.1f us of other kernels in the process left out)'
             % (launches, ns * 1e-3, len(fwd), other * 1e-3), '', '| kernel | launches per forward | us per forward |', '|---|---|---|']
    for r in sorted(fwd, key=lambda r: -float(r['TotalDurationNs']))[:12]:
        lines.append('| `%s` | %d | %.1f |' % (r['Name'][:110], int(r['Calls']) // TRACE_FORWARDS, float(r['TotalDurationNs']) / TRACE_FORWARDS * 1e-3))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stats', default=None)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warm', type=int, default=10)
    ap.add_argument('--config', default='all', choices=['c2', 'c5', 'all'])
    ap.add_argument('--trace', default=None, choices=['b', 'd'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.stats is not None:
        print(stats_summary(a.stats))
        return
    if not torch.cuda.is_available():
        raise SystemExit('infer_timing: needs the GPU (a CPU run gives no time)')
    dev = 'cuda'
    keys = ['c2', 'c5'] if a.config == 'all' else [a.config]
    if a.trace is not None:
        # one variant alone for a kernel trace: 3 eager warm-up forwards + TRACE_REPLAYS replays, all the same launch sequence
        # (TRACE_FORWARDS in all; the collate and the model's construction in front are other kernels, told apart by their names)
        _, B, N, K, T, C = CONFIGS[keys[0]]
        data, net = make(dev, B, N, K, T, C, 500 + N % 89)
        model = net if a.trace == 'b' else InferenceNet(net)
        graph, _ = capture(lambda: model(data))
        for _ in range(TRACE_REPLAYS):
            graph.replay()
        torch.cuda.synchronize()
        print('traced (%s) on %s: %d forwards of one launch sequence' % (a.trace, keys[0], TRACE_FORWARDS))
        return
    text = []
    for key in keys:
        text.append(table(key, time_config(dev, key, a.calls, a.warm), a.calls))
        print(text[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
