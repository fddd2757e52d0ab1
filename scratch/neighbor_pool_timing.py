"""What ops.neighbor_pool (csrc/pool.hip) and models.common.fps_pooling cost against what a user writes without them on the device: the
edge list of the same graph, x[src] materialised per edge, then index_add_ / scatter_reduce_.  profiles/r23_neighbor_pool.md holds what
this prints.

    python scratch/neighbor_pool_timing.py [--out FILE.md]

Shape: 16 x 8192 sources, their fps quarter as targets, K = 16, C in {32, 128}.  Every reduction forward and forward + backward, device
events around 50 back-to-back calls, the op and the framework composition in this one process; algorithmic bytes of a forward = table +
target rows written + source rows once; "bwd launch" is the backward's launch alone (the forward + backward column
is bounded by autograd's host work per call).  fps_pooling against fps -> knn (edge list) -> framework scatter: host clock around the call plus
a device synchronise (both sides read counts back), median (minimum) of 20."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
PEAK_BYTES_PER_S = 8e12
REDUCES = ('sum', 'mean', 'max', 'min')


def events(fn, warm=5, timed=50):
    """Microseconds per call: device events around `timed` back-to-back calls."""
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(timed):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / timed


def wall(fn, warm=3, timed=20):
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
    return '%.3f (%.3f)' % (float(np.median(out)), float(np.min(out)))


def framework_scatter(x, i, j, n_tgt, reduce, deg):
    """scatter(x[j], i, dim=0, reduce=) with framework kernels (atomics): what the parent commit's user writes."""
    import torch
    v = x[j]
    if reduce in ('sum', 'mean'):
        out = torch.zeros((n_tgt, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, i, v)
        return out / deg if reduce == 'mean' else out
    return torch.zeros((n_tgt, x.shape[1]), dtype=x.dtype, device=x.device).scatter_reduce(
        0, i[:, None].expand(-1, x.shape[1]), v, 'amax' if reduce == 'max' else 'amin', include_self=False)


def backward_launch(table, g, reduce, x):
    """The backward launch alone (no autograd around it): us per call over the saved tensors of one forward."""
    import torch
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    code = ops.POOL_REDUCE[reduce]
    C = x.shape[1]
    out = torch.empty((table.m_tgt, C), dtype=torch.float32, device=x.device)
    arg = torch.empty((table.m_tgt, C), dtype=torch.int32, device=x.device)
    count = torch.empty(table.m_tgt, dtype=torch.int32, device=x.device)
    _lib.call('crfconv_neighbor_pool_forward', ptr(x), ptr(table.idx32), table.K, table.m_tgt, C, code, ptr(out), ptr(arg), ptr(count),
              stream_ptr())
    rev_ptr, rev_eid = table.reverse
    dx = torch.empty_like(x)
    if code >= 2:
        return events(lambda: _lib.call('crfconv_neighbor_maxpool_backward', ptr(g), ptr(arg), ptr(rev_ptr), ptr(rev_eid), table.K,
                                        table.m_src, C, ptr(dx), stream_ptr()))
    return events(lambda: _lib.call('crfconv_neighbor_pool_backward', ptr(g), ptr(count) if code == 1 else None, ptr(rev_ptr), ptr(rev_eid),
                                    table.K, table.m_src, C, ptr(dx), stream_ptr()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from benchlib.common import synth_cloud
    from crfconv_amd import ops
    from crfconv_amd.models import common, graph_ops
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev, B, N, K = 'cuda:0', 16, 8192, 16
    pos = torch.from_numpy(np.concatenate([synth_cloud(7000 + b, N)[0] for b in range(B)])).to(dev)
    batch = torch.arange(B, device=dev).repeat_interleave(N)
    idx = graph_ops.fps(pos, batch, 0.25)
    table = graph_ops.knn_table(pos, pos[idx], K, batch, batch[idx])
    edges = graph_ops.knn(pos, pos[idx], K, batch, batch[idx])
    i, j = edges[0].contiguous(), edges[1].contiguous()
    m_tgt, m_src = table.m_tgt, table.m_src
    deg = torch.bincount(i, minlength=m_tgt).clamp_(min=1).to(torch.float32)[:, None]
    rev_ptr, _ = table.reverse
    rlen = (rev_ptr[1:] - rev_ptr[:-1])
    lines = ['command: python scratch/neighbor_pool_timing.py; us per call, device events around 50 back-to-back calls', '',
             '(1) ops.neighbor_pool against x[src] + index_add_ / scatter_reduce_ over the edge list of the same graph: %d sources, %d targets, '
             'K = %d (table width %d, %d edges); reverse rows: median %d, maximum %d edges'
             % (m_src, m_tgt, K, table.K, i.numel(), int(rlen.median()), int(rlen.max())),
             '    %-5s %-5s %12s %12s %14s %14s %16s %10s %12s %10s' % ('C', 'reduce', 'op fwd', 'frame fwd', 'op fwd+bwd', 'frame fwd+bwd',
                                                                       'fwd alg. bytes', 'of 8 TB/s', 'bwd launch', 'same bits')]
    gen = torch.Generator(device=dev).manual_seed(5)
    for C in (32, 128):
        x = torch.randn((m_src, C), device=dev, generator=gen).requires_grad_()
        g = torch.randn((m_tgt, C), device=dev, generator=gen)
        xd = x.detach()
        nbytes = m_tgt * table.K * 4 + m_tgt * C * 4 + m_src * C * 4
        for reduce in REDUCES:
            def op_both():
                x.grad = None
                ops.neighbor_pool(x, table, reduce).backward(g)

            def frame_both():
                x.grad = None
                framework_scatter(x, i, j, m_tgt, reduce, deg).backward(g)
            f_op = events(lambda: ops.neighbor_pool(xd, table, reduce))
            f_fr = events(lambda: framework_scatter(xd, i, j, m_tgt, reduce, deg))
            b_op, b_fr = events(op_both), events(frame_both)
            k_bw = backward_launch(table, g, reduce, xd)
            op_both()
            a, ga = ops.neighbor_pool(xd, table, reduce), x.grad.clone()
            op_both()
            same = torch.equal(a, ops.neighbor_pool(xd, table, reduce)) and torch.equal(ga, x.grad)
            lines.append('    %-5d %-5s %12.1f %12.1f %14.1f %14.1f %16d %10.3f %12.1f %10s'
                         % (C, reduce, f_op, f_fr, b_op, b_fr, nbytes, nbytes / (f_op * 1e-6) / PEAK_BYTES_PER_S, k_bw, same))
    lines += ['', '(2) fps_pooling(pos, x, edge_attr, batch, k = 16, r = 0.25) against fps -> knn edge list -> framework scatter, same shape, '
              'C = 32, 5 edge attributes; ms, median (minimum) of 20, host clock + synchronise']
    x = torch.randn((m_src, 32), device=dev, generator=gen)
    ea = torch.randn((m_src, 5), device=dev, generator=gen)

    def composed(reduce):
        pick = graph_ops.fps(pos, batch, 0.25)
        e = graph_ops.knn(pos, pos[pick], K, batch, batch[pick])
        d = torch.bincount(e[0], minlength=pick.numel()).clamp_(min=1).to(torch.float32)[:, None]
        return framework_scatter(x, e[0], e[1], pick.numel(), reduce, d), pos[pick], ea[pick], batch[pick]
    for reduce in ('sum', 'mean', 'max'):
        lines.append('    %-5s fps_pooling %s   composition %s' % (reduce, wall(lambda: common.fps_pooling(pos, x, ea, batch, K, 0.25, reduce)),
                                                                 wall(lambda: composed(reduce))))
    lines.append('    fps alone %s   (the sequential part both sides share)' % wall(lambda: graph_ops.fps(pos, batch, 0.25)))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
