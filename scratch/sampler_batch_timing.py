"""Timing behind DESIGN 6c: B crops as B x PossibilitySampler.get_random (the one-crop path: host cloud choice, host draws, full sort
of the cloud; wall clock with a final synchronise) against get_batch(B) eagerly and as a graph replay (HIP events), 20 repetitions
after 5 warm-ups, same process, same clouds; and CollateGraph.run() with and without sampler= at 4 x 40 960 points.
Writes $OUT_ROOT/sampler_batch_timing.json (default scratch/out/).  --trace: a few batch calls only (for rocprofv3 --kernel-trace)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crfconv_amd.data import CollateGraph, Data, multiscale_compute      # noqa: E402
from crfconv_amd.sampling import PossibilitySampler                      # noqa: E402

DEV, REPS, WARM = 'cuda', 20, 5


def stats(ms):
    a = np.asarray(ms)
    return {'median_ms': float(np.median(a)), 'min_ms': float(a.min()), 'max_ms': float(a.max()),
            'iqr_ms': float(np.percentile(a, 75) - np.percentile(a, 25))}


def events(fn):
    out = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARM:
            out.append(a.elapsed_time(b))
    return stats(out)


def wall(fn):
    out = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def sampler(n, k, seed=3):
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=gen) * torch.tensor([60.0, 60.0, 15.0])).to(DEV)
    rgb = torch.rand(n, 3, generator=gen).to(DEV)
    labels = torch.randint(0, 8, (n,), generator=gen).to(DEV)
    return PossibilitySampler([pts], rgb=[rgb], labels=[labels], num_points=k, class_weight=np.linspace(0.5, 2.0, 8), generator=gen)


def one_size(n, k, B):
    smp = sampler(n, k)
    res = {'n': n, 'k': k, 'B': B}
    res['get_random_loop_wall'] = wall(lambda: [smp.get_random() for _ in range(B)])
    res['get_batch_eager_events'] = events(lambda: smp.get_batch(B))
    res['get_batch_eager_wall'] = wall(lambda: smp.get_batch(B))
    out = Data(pos=torch.empty((B, k, 3), device=DEV), x=torch.empty((B, k, 6), device=DEV),
               y=torch.empty((B, k), dtype=torch.int64, device=DEV), point_idx=torch.empty((B, k), dtype=torch.int64, device=DEV),
               cloud_idx=torch.empty((B, 1), dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        smp.get_batch(B, out=out)
    res['get_batch_replay_events'] = events(graph.replay)
    res['get_batch_replay_wall'] = wall(graph.replay)
    return res


def collate(B=4, N=40960, n=1 << 20):
    smp = sampler(n, N)

    def static():
        d = smp.get_batch(B)
        return multiscale_compute(d.pos, x=d.x, y=d.y, point_idx=d.point_idx, cloud_idx=d.cloud_idx, generator=torch.Generator().manual_seed(1))
    d = smp.get_batch(B)
    plain = CollateGraph(static(), generator=torch.Generator().manual_seed(2))
    drawn = CollateGraph(static(), generator=torch.Generator().manual_seed(2), sampler=smp)
    plain_in = (d.pos, d.x, d.y)
    plain.target.point_idx = plain.target.cloud_idx = None
    plain.run(*plain_in)
    drawn.run()
    return {'B': B, 'N': N, 'n': n, 'collate_run_given_clouds_wall': wall(lambda: plain.run(*plain_in)),
            'collate_run_sampler_wall': wall(drawn.run),
            'collate_run_given_clouds_events': events(lambda: plain.run(*plain_in)), 'collate_run_sampler_events': events(drawn.run)}


if __name__ == '__main__':
    if '--trace' in sys.argv:
        smp = sampler(1 << 20, 65536)
        for _ in range(3):
            smp.get_batch(4)
        torch.cuda.synchronize()
        sys.exit(0)
    res = {'sizes': [one_size(1 << 20, 65536, 16), one_size(1 << 20, 40960, 4)], 'collate': collate()}
    out_root = os.environ.get('OUT_ROOT', os.path.join(ROOT, 'scratch', 'out'))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, 'sampler_batch_timing.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
