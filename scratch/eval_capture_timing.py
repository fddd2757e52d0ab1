"""What the self-capturing eval forward and the fused classifier head buy, in one process.  profiles/r13_eval_capture.md holds what
this prints.

    python scratch/eval_capture_timing.py [--tree DIR] [--what call|head|all] [--out FILE.md]

(1) The reference's validation call -- ``with torch.no_grad(): model(data)`` on the bare eval-mode PointConvBig (trainval.py:110-124)
    -- at BASELINE config 2 (4 x 40 960 points, K 16, CRF decoders, T 3, 13 classes; the synthetic clouds of bench.py): per call the
    time between two HIP events around it AND the host's wall clock from before the call to after a device synchronisation, with
    the model's own capture on and off.  --tree DIR imports crfconv_amd from another checkout (built there): on a tree from before
    the eval capture both legs are the eager call, which is the comparison the feature has to win.
(2) The classifier head at M = 163 840, Ci = 32, 13 classes, three forms: ops.head_eval; linear_bn_act + ops.linear;
    crfconv_head_forward(p = 0) with a mask buffer (the training kernel).  HIP events around every call.

Protocol: 5 warm-up calls, 20 timed ones, median and minimum."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TIMED = 5, 20


def timed(fn, wall=False):
    """(event ms [TIMED], wall ms [TIMED] or None): every call between two HIP events; wall: host clock around call + synchronise."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev, wl = [], []
    for _ in range(TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wl.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return ev, (wl if wall else None)


def row(name, ev, wl=None):
    cells = '| %s | %.4f | %.4f |' % (name, float(np.median(ev)), float(np.min(ev)))
    return cells + (' %.4f | %.4f |' % (float(np.median(wl)), float(np.min(wl))) if wl is not None else '')


def validation_call(dev):
    import crfconv_amd
    from benchlib.common import synth_cloud
    from crfconv_amd import models, train
    B, N, K, T, C = 4, 40960, 16, 3, 13

    def batch(seed):
        clouds = [synth_cloud(seed + i, N) for i in range(B)]
        pos = torch.from_numpy(np.stack([c[0] for c in clouds])).to(dev)
        x = torch.cat([pos, torch.from_numpy(np.stack([c[1] for c in clouds])).to(dev)], -1)
        return crfconv_amd.multiscale_compute(pos, x=x, kernel_size=(K,) * 5, generator=torch.Generator().manual_seed(seed), sort='morton')
    data = [batch(500), batch(600)]                        # a validation loop hands over another batch at every call
    torch.manual_seed(7)
    net = models.PointConvBig(6, C, use_crf=True, steps=T).to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    net.eval()
    has_capture = hasattr(train, 'GraphedInference')
    turn = [0]

    def call():
        turn[0] += 1
        with torch.no_grad():
            return net(data[turn[0] % 2])
    lines = ['### The validation call: `with torch.no_grad(): model(data)`, 4 x 40 960 points, K = 16, T = 3, 13 classes', '',
             'tree: %s (%s the eval capture)' % (os.path.abspath(TREE), 'with' if has_capture else 'WITHOUT'), '',
             '%d warm-up calls, %d timed; two batches alternate' % (WARM, TIMED), '',
             '| leg | HIP events: median ms | min ms | wall incl. synchronise: median ms | min ms |', '|---|---|---|---|---|']
    for on in (False, True):
        train.set_autograph(on)
        ev, wl = timed(call, wall=True)
        lines.append(row('autograph %s' % ('on' if on else 'off'), ev, wl))
    if has_capture:
        st = train.stats(net)['eval']
        lines += ['', 'stats(model)[eval] afterwards: captures %d, replays %d, eager %s' % (st['captures'], st['replays'], dict(st['eager']))]
        with torch.no_grad():
            a = net(data[0]).clone()
            with train.no_autograph():
                b = net(data[0])
        lines += ['', 'replayed logits torch.equal to the eager ones: %s' % bool(torch.equal(a, b))]
    return '\n'.join(lines)


def head(dev):
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    if not hasattr(ops, 'head_eval'):
        return '### The classifier head\n\nthis tree has no ops.head_eval'
    M, Ci, Co, C2, slope = 163840, 32, 128, 13, 0.1
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(M, Ci, generator=g) * 2 - 1).to(dev)
    W1 = ((torch.rand(Co, Ci, generator=g) * 2 - 1) * 0.3).to(dev)
    W2 = ((torch.rand(C2, Co, generator=g) * 2 - 1) * 0.3).to(dev)
    b2 = (torch.rand(C2, generator=g) - 0.5).to(dev)
    bn = torch.nn.BatchNorm1d(Co).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    coef = ops.bn_eval_coefs([bn])[1][0]
    logits = torch.empty((M, C2), device=dev)
    mask = torch.empty(_lib.load().crfconv_head_mask_words(M), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def fused():
        return ops.head_eval(x, W1, coef, slope, W2, b2)

    def two(min_rows):
        def run():
            prev, ops.state.mfma_min_rows = ops.state.mfma_min_rows, (min_rows if min_rows is not None else ops.state.mfma_min_rows)
            try:
                with torch.no_grad():
                    return ops.linear(ops.linear_bn_act(x, W1, coef, slope=slope), W2, b2)
            finally:
                ops.state.mfma_min_rows = prev
        return run

    def training_kernel():
        _lib.call('crfconv_head_forward', ptr(x), ptr(W1), ptr(coef), slope, 0.0, 1, ptr(counter), ptr(W2), ptr(b2), M, Ci, Co, C2,
                  ptr(logits), ptr(mask), None, stream_ptr())
        return logits
    ref = fused()
    lines = ['### The classifier head: M = 163 840, 32 -> 128 -> 13', '', '%d warm-up calls, %d timed, HIP events around every call' % (WARM, TIMED),
             '', '| form | median ms | min ms |', '|---|---|---|']
    lines.append(row('`ops.head_eval` (one launch, no [M, 128] tensor)', timed(fused)[0]))
    lines.append(row('`linear_bn_act` + `ops.linear` (default state)', timed(two(None))[0]))
    lines.append(row('`crfconv_head_forward(p = 0)` with a mask (the training kernel)', timed(training_kernel)[0]))
    lines += ['', 'head_eval torch.equal to crfconv_head_forward(p = 0) with a mask: %s' % bool(torch.equal(ref, training_kernel()))]
    for mr, name in ((None, 'the default state'), (1, 'min_rows(1)')):
        other = two(mr)()
        lines.append('head_eval torch.equal to linear_bn_act + linear in %s: %s (max |difference| %.3e, max |logit| %.3e)'
                     % (name, bool(torch.equal(ref, other)), float((ref - other).abs().max()), float(other.abs().max())))
    return '\n'.join(lines)


def main():
    global TREE
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=HERE, help='checkout to import crfconv_amd (and benchlib) from; default: this one')
    ap.add_argument('--what', default='all', choices=['call', 'head', 'all'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    TREE = a.tree
    sys.path.insert(0, os.path.abspath(TREE))
    if not torch.cuda.is_available():
        raise SystemExit('eval_capture_timing: needs the GPU (a CPU run gives no time)')
    text = []
    if a.what in ('call', 'all'):
        text.append(validation_call('cuda'))
        print(text[-1], flush=True)
        torch.cuda.empty_cache()
    if a.what in ('head', 'all'):
        text.append(head('cuda'))
        print(text[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n\n'.join(text) + '\n')


TREE = HERE

if __name__ == '__main__':
    main()
