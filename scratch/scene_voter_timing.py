"""Tiled-scene inference on the C5-like scene of benchlib/configs.py (1 048 576 points, crops of 65 536, K = 32, T = 5, 8 classes): the
cached graphed path of ``vote_scene`` (graph_cache with the graphs already captured: one device -> host read free -- a single cloud --
but per crop a host-side get_random, three copies, two replays and a per-sample vote call) against ``SceneVoter`` at B = 1, 2, 4
(two replays per batch).  profiles/r9_scene_voter.md holds the table this prints.

    python scratch/scene_voter_timing.py [--crops 32] [--reps 7] [--out FILE.md]

Per repetition every arm votes `crops` crops; device events around the loop, a device synchronise behind it; the arms alternate within
one process (their order rotates from repetition to repetition); scene points per second = crops x 65 536 / time.  The first two
SceneVoter steps (eager + capture of forward and votes; capture of the collate graph) are timed apart, by the host clock."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from crfconv_amd import models                                                          # noqa: E402
from crfconv_amd.sampling import PossibilitySampler, SceneVoter, VoteAccumulator, vote_scene      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crops', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--points', type=int, default=1 << 20)
    ap.add_argument('--crop-points', type=int, default=65536)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = 'cuda'
    K, T, C = 32, 5, 8
    g = torch.Generator().manual_seed(50)
    pts = (torch.rand(a.points, 3, generator=g) * torch.tensor([60.0, 60.0, 15.0])).to(dev)
    rgb = torch.rand(a.points, 3, generator=g).to(dev)
    torch.manual_seed(50)
    net = models.PointConvBig(6, C, use_crf=True, steps=T).to(dev).eval()

    def sampler():
        return PossibilitySampler([pts], rgb=[rgb], num_points=a.crop_points, split='test', generator=torch.Generator().manual_seed(51))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the parent's best path: the graphs of the crop shape captured once, kept across scenes
    cache = {}
    parent_votes = VoteAccumulator([a.points], C, device=dev)
    vote_scene(sampler(), net, parent_votes, 3, kernel_size=(K,) * 5, generator=torch.Generator().manual_seed(52), graphed=True, graph_cache=cache)
    parent_smp = sampler()                                   # one sampler per arm, continued from repetition to repetition

    def parent():
        vote_scene(parent_smp, net, parent_votes, a.crops, kernel_size=(K,) * 5, generator=torch.Generator().manual_seed(52), graphed=True,
                   graph_cache=cache)
    arms = {'vote_scene(graphed, cached)': parent}
    first = {}
    for B in (1, 2, 4):
        if a.crops % B:
            raise SystemExit('--crops must be a multiple of 4')
        voter = SceneVoter(sampler(), net, VoteAccumulator([a.points], C, device=dev), B, kernel_size=(K,) * 5,
                           generator=torch.Generator().manual_seed(52))
        steps = []
        for _ in range(3):                                   # step 1: eager + capture; step 2: capture of the collate graph; step 3: replays
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            voter.step()
            torch.cuda.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3)
        first['B = %d' % B] = steps
        arms['SceneVoter B = %d' % B] = (lambda v=voter, n=a.crops // B: v.run(n_batches=n))
    for fn in arms.values():                                 # warm-up of every arm at the timed length
        fn()
    torch.cuda.synchronize()
    names = list(arms)
    ms = {n: [] for n in names}
    for rep in range(a.reps):
        for i in range(len(names)):
            n = names[(i + rep) % len(names)]
            ms[n].append(timed(arms[n]))
    parent_votes.check()
    crop_points = a.crops * a.crop_points
    rows = []
    for n in names:
        v = sorted(ms[n])
        med = v[len(v) // 2]
        rows.append({'arm': n, 'median_ms': med, 'min_ms': v[0], 'max_ms': v[-1], 'ms_per_crop': med / a.crops,
                     'scene_points_per_s_M': crop_points / med / 1e3, 'all_ms': ms[n]})
    lines = ['| arm | median ms / %d crops | min | max | spread (max - min) / median | ms per crop | M scene points / s |' % a.crops,
             '|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append('| `%s` | %.2f | %.2f | %.2f | %.1f %% | %.3f | %.2f |' % (r['arm'], r['median_ms'], r['min_ms'], r['max_ms'],
                                                                              100 * (r['max_ms'] - r['min_ms']) / r['median_ms'], r['ms_per_crop'],
                                                                              r['scene_points_per_s_M']))
    lines += ['', '| SceneVoter | step 1 (eager + capture) ms | step 2 (collate graph capture) ms | step 3 (two replays) ms |', '|---|---|---|---|']
    for n, s in first.items():
        lines.append('| %s | %.1f | %.1f | %.2f |' % (n, s[0], s[1], s[2]))
    text = '\n'.join(lines)
    print(text)
    print(json.dumps({'crops': a.crops, 'reps': a.reps, 'scene_points': a.points, 'crop_points': a.crop_points, 'K': K, 'T': T, 'classes': C,
                      'rows': rows, 'first_steps_ms': first}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
