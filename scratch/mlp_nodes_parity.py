"""Same launches, same bits: the fused MLP nodes of ops.mlp under one Python package against another, on ONE built library.

    CRFCONV_LIB=<lib> python scratch/mlp_nodes_parity.py run --pkg <checkout root> --out a.pt      # once per package (parent twice)
    python scratch/mlp_nodes_parity.py compare parent_1.pt parent_2.pt tree.pt

`run` imports crfconv_amd from `--pkg` (default: this tree), wraps _lib.call, and records for every family of
tests/test_gpu_mlp_nodes.py and for one eager training step of PointConvBig(6, 13, use_crf=True, steps=2) on two 4096-point clouds
(row-streaming forms from 4096 rows), each in the three delivery modes of the parameter gradients: the library calls in order with
their non-pointer arguments, and outputs, input gradients, parameter gradients and BatchNorm buffers.  `compare` demands identical call
lists, torch.equal for every tensor the first package reproduces between its own two runs, and for the others a difference within that
run-to-run difference (profiles/r11_mlp_nodes.md)."""
import argparse
import ctypes
import os
import sys

os.environ.setdefault('CRFCONV_AUTOGRAPH', '0')
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def record_calls(_lib, log):
    real = _lib.call

    def call(name, *args):
        types = _lib.SIGNATURES[name][1]
        log.append((name,) + tuple(a for a, t in zip(args, types) if t is not ctypes.c_void_p and isinstance(a, (int, float, bool))))
        return real(name, *args)
    _lib.call = call


def run(pkg, out):
    for p in (os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests'), pkg):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import crfconv_amd
    from crfconv_amd import _lib, distributed, models, ops, train
    import _seeded as S
    import test_gpu_mlp_nodes as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(crfconv_amd.__file__))) == os.path.abspath(pkg), crfconv_amd.__file__
    ops.state.mfma_min_rows = 4096
    log = []
    record_calls(_lib, log)
    calls, tensors = {}, {}
    for name in T.FAMILIES:
        case = T.build_family(name)
        for mode in T.MODES:
            del log[:]
            res = T.run_family(case, mode)
            calls['%s/%s' % (name, mode)] = list(log)
            assert T.FAMILIES[name][1] in res['nodes']
            for grp in ('same', 'pgrad'):
                for k, v in res[grp].items():
                    tensors['%s/%s/%s' % (name, mode, k)] = v.cpu()
    # one eager training step of the whole network
    B, N = 2, 4096
    pos = np.stack([S.make_cloud(95 + b, N, box=(2, 2, 1)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(95, 'rgb', (B, N, 3), 0, 1)], -1)
    data = crfconv_amd.multiscale_compute(torch.from_numpy(pos).to(T.DEV), torch.from_numpy(feats).to(T.DEV),
                                          generator=torch.Generator().manual_seed(5))
    labels = torch.from_numpy(S.integers(95, 'y', (B, N), 0, 14)).to(T.DEV)
    torch.manual_seed(3)
    net = models.PointConvBig(6, 13, use_crf=True, steps=2).to(T.DEV).train()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    bucket = distributed.FlatGradAllReduce(net)
    for mode in T.MODES:
        torch.manual_seed(7)
        net.load_state_dict(sd)
        bucket.zero()
        del log[:]
        with train.no_autograph():
            logits = net(data)
            loss = ops.training_loss(logits, labels, None, ignore_index=-1)
            if mode == 'autograd':
                loss.backward()
            else:
                with ops.deferred_weight_grads(sink=bucket.view_of if mode == 'bucket' else None):
                    loss.backward()
        torch.cuda.synchronize()
        calls['net/%s' % mode] = list(log)
        tensors['net/%s/logits' % mode] = logits.detach().cpu()
        tensors['net/%s/loss' % mode] = loss.detach().cpu()
        for k, p in net.named_parameters():
            if p.grad is not None:
                tensors['net/%s/grad/%s' % (mode, k)] = p.grad.detach().cpu().clone()
        for k, v in net.state_dict().items():
            if 'running' in k or 'num_batches' in k:
                tensors['net/%s/buf/%s' % (mode, k)] = v.detach().cpu().clone()
    assert int(ops.gridsync_ws(T.DEV).abs().sum()) == 0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    torch.save({'calls': calls, 'tensors': tensors}, out)
    print('%s: %d call lists (%d calls), %d tensors' % (out, len(calls), sum(len(v) for v in calls.values()), len(tensors)))


def compare(first, second, other):
    import torch
    a, a2, b = (torch.load(p) for p in (first, second, other))
    bad = 0
    for k in sorted(set(a['calls']) | set(b['calls'])):
        if a['calls'].get(k) != b['calls'].get(k) or a['calls'].get(k) != a2['calls'].get(k):
            bad += 1
            print('CALLS DIFFER', k)
    print('call lists: %d, %d calls, differing: %d' % (len(a['calls']), sum(len(v) for v in a['calls'].values()), bad))
    noisy = []
    assert a['tensors'].keys() == a2['tensors'].keys() == b['tensors'].keys()
    for k, v in a['tensors'].items():
        if torch.equal(v, a2['tensors'][k]):
            if not torch.equal(v, b['tensors'][k]):
                bad += 1
                print('TENSOR DIFFERS', k, float((v.double() - b['tensors'][k].double()).abs().max()))
        else:
            own = float((v.double() - a2['tensors'][k].double()).abs().max())
            d = min(float((w.double() - b['tensors'][k].double()).abs().max()) for w in (v, a2['tensors'][k]))
            noisy.append((k, own, d))
            if d > own:
                bad += 1
                print('TENSOR OUTSIDE THE RUN-TO-RUN DIFFERENCE', k, own, d)
    print('tensors: %d, not reproduced by the first package itself: %d' % (len(a['tensors']), len(noisy)))
    for k, own, d in noisy:
        print('  %-70s own run-to-run %.3e   against the other %.3e' % (k, own, d))
    print('PARITY %s' % ('FAILED' if bad else 'OK'))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--pkg', default=ROOT)
    r.add_argument('--out', required=True)
    c = sub.add_parser('compare')
    c.add_argument('files', nargs=3)
    args = ap.parse_args()
    sys.exit(run(os.path.abspath(args.pkg), args.out) if args.cmd == 'run' else compare(*args.files))
