"""Host cost of the per-call checks of the self-capturing model (train.GraphedModel.forward / autograph_forward): what a replayed step
pays on top of the replays for noticing hooks, re-homed parameters / buffers and frozen parameters, against the walk over
model.parameters() the frozen check used to make.  Needs no GPU: a CPU-built PointConvBig, the runner's capture-time snapshot only.
usage: python3 scratch/autograph_host_cost.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crfconv_amd import models, train

net = models.PointConvBig(6, 13, use_crf=True, steps=3).train()
runner = train.GraphedModel(net, guard_pending=True)
runner._snapshot()
runner.fwd_graph = object()                          # (as after a capture: hooked() reads the snapshot)
print('%d parameters, %d buffers, %d modules' % (len(list(net.parameters())), len(list(net.buffers())), len(list(net.modules()))))


def per_call(fn, n=2000):
    for _ in range(200):
        fn()
    best = float('inf')
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        best = min(best, (time.perf_counter() - t0) / n)
    return best * 1e6


def added():
    assert not runner.hooked()
    assert not runner._moved()
    assert [p.requires_grad for p in runner._all_params] == runner._grad_flags


rows = [('hooked() (every module\'s hook dicts + global hooks)', runner.hooked),
        ('_moved() (slot identities + data_ptr of params / buffers)', runner._moved),
        ('requires_grad flags', lambda: [p.requires_grad for p in runner._all_params] == runner._grad_flags),
        ('all checks added per replayed step', added),
        ('before: frozen check via model.parameters()', lambda: tuple(p.requires_grad for p in net.parameters()))]
for what, fn in rows:
    print('%-56s %7.1f us' % (what, per_call(fn)))
