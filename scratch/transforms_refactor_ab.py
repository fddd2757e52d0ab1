"""Parent against new for the transforms refactor (one chain behind Compose and SegmentCompose, the spec check and the per-point steps in
csrc/augment_common.hpp): the same bits out of every call, and the same speed.  profiles/r29_transforms_refactor.md holds what this prints.

    python scratch/transforms_refactor_ab.py --what bits|timing|bench|all --parent DIR [--out FILE.md] [--out-dir DIR]
    python scratch/transforms_refactor_ab.py --leg bits|timing [--tree DIR] --file FILE      # one side, one process (started by the above)

DIR is a checkout of the parent commit, built there.  One child process per side imports crfconv_amd from its own tree.

bits    every output tensor of: dense apply_batch (B in {1, 3}, N in {1, 5, 1024, 1027, 4100}, x none / C = 3 / C = 6, the trainval chain with
        RandomSymmetry on all axes and without symmetry, drawn and given parameters and noise); Compose.__call__ on 2048 points with rgb, with
        and without AddFeatsByKeys(delete_feats=[False, True]); apply_segments on clouds of SIZES at row 0 and one row further in (four
        layouts, three chains, drawn and given); SegmentCompose.__call__ with FixedPoints in its three modes, num in {1, 64, 2048}.  Written
        to one .npz per side and compared with array_equal on the CPU.
timing  us per call between two device events around 50 back-to-back calls, five windows after 10 calls: dense apply_batch at 4 x 40 960,
        apply_segments at 16 x 8192 and at the uneven 16-cloud split, the three pick modes at 16 x 8192; wall us per call of Compose.__call__
        and SegmentCompose.__call__, 200 calls after 20 with one synchronise at the end, seven windows.  Fresh processes: parent, new, parent,
        new.  The yardstick is the span of the parent's own windows.
bench   bench.py --gpus 1 --steps 100 --warmup 10 in each tree, parent, new, parent, new: ms_per_step and final_loss."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 0, 63, 64, 65, 1023, 1024, 1025, 4097]        # the empty cloud, partial lane groups, the walk above 4096
UNEVEN = [1, 37, 512, 1000, 2048, 3000, 4096, 4097, 6000, 8192, 9000, 12000, 16384, 20000, 24000]      # + the rest: 16 clouds, 131 072 rows
SEED, COUNTER = 20240607, 7
SENTINEL = -12345.0


def augmentation(T, symmetry=True, sigma=0.01):
    steps = [T.RandomRotate(180, axis=2), T.RandomScaleAnisotropic([0.8, 1.2])]
    if symmetry:
        steps.append(T.RandomSymmetry([True, True, True]))
    return steps + [T.RandomNoise(sigma=sigma, clip=0.05)]


def given_params(rng, S):
    th = rng.uniform(-np.pi, np.pi, S)
    p = np.zeros((S, 8), np.float32)
    p[:, 0], p[:, 1], p[:, 2:5] = np.cos(th), np.sin(th), rng.uniform(0.8, 1.2, (S, 3))
    p[:, 5], p[:, 6] = (3 * np.arange(S) + 5) % 8, np.arange(S) % 2
    return p


def leg_bits(dev):
    import torch
    from crfconv_amd import transforms as T
    from crfconv_amd.data import Data
    out = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def keep(key, **tensors):
        for name, v in tensors.items():
            if v is not None:
                out['%s/%s' % (key, name)] = v.cpu().numpy()

    def gen():
        return torch.Generator().manual_seed(1)
    counter = torch.full((1,), COUNTER, dtype=torch.int64, device=dev)
    add_rgb = T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[False, True])
    # ---- dense apply_batch
    for sym in (True, False):
        chain = T.Compose(augmentation(T, sym) + [T.DropFeature(0.2, 'rgb'), add_rgb], generator=gen())
        for B in (1, 3):
            for N in (1, 5, 1024, 1027, 4100):
                rng = np.random.default_rng(10000 * B + N)
                pos0 = (rng.uniform(-1, 1, (B, N, 3)) * [3, 2, 1]).astype(np.float32)
                rgb0 = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
                noise0 = rng.uniform(-0.1, 0.1, (B, N, 3)).astype(np.float32)
                params0 = given_params(rng, B)
                for C in (0, 3, 6):
                    for how in ('drawn', 'given'):
                        pos = t(pos0)
                        x = None if C == 0 else t(np.concatenate([pos0 * 0 + 7] + ([rgb0] if C == 6 else []), -1))
                        pout = torch.full((B, 8), -7.0, device=dev)
                        extra = {'params_in': t(params0), 'noise_in': t(noise0)} if how == 'given' else {}
                        chain.apply_batch(pos, x, SEED, counter, params_out=pout, **extra)
                        keep('apply_batch/sym%d/B%d/N%d/C%d/%s' % (sym, B, N, C, how), pos=pos, x=x, params_out=pout)
    # ---- dense Compose.__call__
    rng = np.random.default_rng(2048)
    pos0 = (rng.uniform(-1, 1, (2048, 3)) * [3, 2, 1]).astype(np.float32)
    rgb0 = rng.uniform(0, 1, (2048, 3)).astype(np.float32)
    for add in (True, False):
        chain = T.Compose(augmentation(T) + [T.DropFeature(0.2, 'rgb')] + ([add_rgb] if add else []), generator=gen())
        chain.load_state_dict({'seed': SEED, 'counter': COUNTER})
        for call in range(6):                                    # (six counters: kept and dropped rgb both occur)
            data, pout = Data(pos=t(pos0), rgb=t(rgb0)), torch.full((8,), -7.0, device=dev)
            data = chain(data, params_out=pout)
            key = 'Compose.__call__/add%d/call%d' % (add, call)
            keep(key, pos=data.pos, rgb=getattr(data, 'rgb', None), x=getattr(data, 'x', None), params_out=pout)
            out[key + '/attributes'] = np.array(sorted(k for k, v in data.__dict__.items() if v is not None))
        out['Compose.__call__/add%d/counter' % add] = np.array(chain.state_dict()['counter'])
    # ---- ragged apply_segments
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    S, N = len(SIZES), int(ptr[-1])
    rng = np.random.default_rng(3)
    off = rng.uniform(-400, 400, (S, 3))
    pos0 = np.concatenate([rng.uniform(-1, 1, (n, 3)) * [3, 2, 1] + off[b] for b, n in enumerate(SIZES)]).astype(np.float32)
    nrm = rng.standard_normal((N, 3))
    norm0 = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    norm0[[2, 70, N - 1]] = 0
    rgb0 = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    noise0 = rng.uniform(-0.1, 0.1, (N, 3)).astype(np.float32)
    params0 = given_params(rng, S)

    def rows(a, lead):                                           # (buffer of sentinels, view of rows lead ..): what lies around is compared too
        buf = torch.full((lead + a.shape[0] + 3, a.shape[1]), SENTINEL, device=dev)
        view = buf[lead:lead + a.shape[0]]
        view.copy_(t(a))
        return buf, view
    for lead in (0, 1):
        for layout in ('pos_norm', 'pos_rgb', 'pos', None):
            for kind in ('normalize+augmentation', 'center', 'augmentation'):
                steps = {'normalize+augmentation': [T.NormalizeScale()] + augmentation(T, sigma=0.03), 'center': [T.Center()],
                         'augmentation': augmentation(T, sigma=0.03)}[kind]
                if layout == 'pos_rgb':
                    steps += ([] if kind == 'center' else [T.DropFeature(0.2)]) + [T.AddFeatsByKeys([True, True], ['pos', 'rgb'])]
                elif layout == 'pos_norm':
                    steps += [T.AddFeatsByKeys([True, True], ['pos', 'norm'])]
                elif layout == 'pos':
                    steps += [T.AddFeatsByKeys([True], ['pos'])]
                chain = T.SegmentCompose(steps, generator=gen())
                for how in ('drawn', 'given'):
                    pbuf, pos = rows(pos0, lead)
                    nbuf, norm = rows(norm0, lead) if layout in ('pos_norm', None) else (None, None)
                    xbuf = x = None
                    if layout == 'pos_rgb':
                        xbuf, x = rows(np.concatenate([pos0 * 0 + 7, rgb0], 1), lead)
                    elif layout is not None:
                        xbuf, x = rows(np.full((N, 6 if layout == 'pos_norm' else 3), 7, np.float32), lead)
                    pout, sout = torch.full((S, 8), -7.0, device=dev), torch.full((S, 4), -7.0, device=dev)
                    extra = {}
                    if how == 'given':
                        extra = {'params_in': t(params0), 'noise_in': rows(noise0, lead)[1]}
                    chain.apply_segments(pos, norm, x, t(ptr), SEED, counter, params_out=pout, stats_out=sout, **extra)
                    keep('apply_segments/lead%d/%s/%s/%s' % (lead, layout, kind, how), pos=pbuf, norm=nbuf, x=xbuf, params_out=pout,
                         stats_out=sout)
    # ---- SegmentCompose.__call__ with FixedPoints
    y0, category0 = np.arange(N, dtype=np.int64), np.arange(S, dtype=np.int64) + 100
    for mode in ('replace', 'subset', 'duplicates'):
        for num in (1, 64, 2048):
            fixed = T.FixedPoints(num, replace=mode == 'replace', allow_duplicates=mode == 'duplicates')
            for rest in ('alone', 'part'):                       # the picks alone; and ahead of the ShapeNet-Part chain, x = [pos, norm]
                tail = [] if rest == 'alone' else ([T.NormalizeScale()] + augmentation(T, sigma=0.001)
                                                   + [T.AddFeatsByKeys([True, True], ['pos', 'norm'])])
                chain = T.SegmentCompose([fixed] + tail, generator=gen())
                chain.load_state_dict({'seed': SEED, 'counter': COUNTER})
                data = Data(pos=t(pos0), norm=t(norm0), y=t(y0), ptr=t(ptr), category=t(category0))
                if mode == 'subset':
                    data.sizes = list(SIZES)
                pout, sout = torch.full((S, 8), -7.0, device=dev), torch.full((S, 4), -7.0, device=dev)
                data = chain(data, params_out=pout, stats_out=sout)
                key = 'SegmentCompose.__call__/%s/num%d/%s' % (mode, num, rest)
                keep(key, pos=data.pos, norm=data.norm, y=data.y, x=getattr(data, 'x', None), ptr=data.ptr, batch=data.batch,
                     category=data.category, params_out=pout, stats_out=sout)
                out[key + '/attributes'] = np.array(sorted(k for k, v in data.__dict__.items() if v is not None))
    torch.cuda.synchronize()
    return out


def leg_timing(dev):
    import torch
    from crfconv_amd import transforms as T
    from crfconv_amd.data import Data
    res = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def events(launch, reset=None, calls=50, times=5, warm=10):
        for _ in range(warm):
            launch()
        got = []
        for _ in range(times):
            if reset is not None:
                reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                launch()
            e1.record()
            e1.synchronize()
            got.append(float(e0.elapsed_time(e1) / calls * 1e3))
        return got

    def wall(call, calls=200, times=7, warm=20):
        for _ in range(warm):
            call()
        got = []
        for _ in range(times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            got.append((time.perf_counter() - t0) / calls * 1e6)
        return got
    rng = np.random.default_rng(0)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    add_rgb = T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[False, True])
    # dense: 4 x 40 960, the trainval chain, x = [pos, rgb]
    dense = T.Compose(augmentation(T) + [T.DropFeature(0.2, 'rgb'), add_rgb], generator=torch.Generator().manual_seed(1))
    pos0 = t((rng.uniform(-1, 1, (4, 40960, 3)) * [3, 2, 1]).astype(np.float32))
    pos, x = pos0.clone(), torch.cat([pos0, t(rng.uniform(0, 1, (4, 40960, 3)).astype(np.float32))], -1).contiguous()
    res['apply_batch 4 x 40960, us'] = events(lambda: dense.apply_batch(pos, x, dense.seed, counter), reset=lambda: pos.copy_(pos0))
    # ragged: the chain and the shapes of profiles/r24_segment_transforms.md
    for name, sizes in (('16 x 8192', [8192] * 16), ('16 uneven', UNEVEN + [131072 - sum(UNEVEN)])):
        S, N = len(sizes), sum(sizes)
        ptr = t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        spos = t((rng.uniform(-1, 1, (N, 3)) * [3, 2, 1] + 200).astype(np.float32))
        nrm = rng.standard_normal((N, 3))
        snorm = t((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32))
        chain = T.SegmentCompose([T.NormalizeScale(), T.RandomRotate(180, axis=2), T.RandomScaleAnisotropic([0.8, 1.2]),
                                  T.RandomSymmetry([True, False, False]), T.RandomNoise(0.01), T.AddFeatsByKeys([True, True], ['pos', 'norm'])],
                                 generator=torch.Generator().manual_seed(1))
        host = chain.draws(chain.seed, 0, S)['params']
        host[:, 5] = 1
        params, sx = t(host), torch.empty((N, 6), device=dev)
        p, n = spos.clone(), snorm.clone()
        res['apply_segments %s, us' % name] = events(lambda: chain.apply_segments(p, n, sx, ptr, chain.seed, counter, params_in=params))
        if name != '16 x 8192':
            continue
        for mode, fixed in (('replace', T.FixedPoints(2048)), ('subset', T.FixedPoints(2048, replace=False)),
                            ('duplicates', T.FixedPoints(2048, replace=False, allow_duplicates=True))):
            pick = T.SegmentCompose([fixed], generator=torch.Generator().manual_seed(2))
            out_host = np.concatenate([[0], np.cumsum(fixed.counts(sizes))]).astype(np.int64)
            out_ptr, M = t(out_host), int(out_host[-1])
            res['picks %s 16 x 8192, us' % mode] = events(lambda: pick.pick(ptr, out_ptr, N, M, pick.seed, counter))
        # the host-bound paths: wall time per whole call
        part = T.SegmentCompose([T.FixedPoints(2048, replace=False, allow_duplicates=True), T.NormalizeScale()] + augmentation(T, sigma=0.001)
                                + [T.AddFeatsByKeys([True, True], ['pos', 'norm'])], generator=torch.Generator().manual_seed(3))
        y = torch.arange(N, device=dev)
        res['SegmentCompose.__call__ 16 x 8192, wall us'] = wall(lambda: part(Data(pos=spos, norm=snorm, y=y, ptr=ptr)))
    one, rgb = pos0[0].clone(), x[0, :, 3:].clone()
    res['Compose.__call__ 40960, wall us'] = wall(lambda: dense(Data(pos=one, rgb=rgb)))
    return res


def child(leg, tree, path, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--file', path] + (['--tree', tree] if tree else [])
    p = subprocess.run(cmd, timeout=timeout)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all', 'bits', 'timing', 'bench'])
    ap.add_argument('--parent', default=None, help='the checkout of the parent commit, built there')
    ap.add_argument('--out', default=None, help='the report (markdown lines)')
    ap.add_argument('--out-dir', default=os.path.join(HERE, 'scratch', 'out', 'transforms_refactor_ab'))
    ap.add_argument('--leg', default=None, choices=['bits', 'timing'], help='one side, in this process')
    ap.add_argument('--tree', default=None, help='--leg: import crfconv_amd from this checkout')
    ap.add_argument('--file', default=None, help='--leg: where the result goes')
    args = ap.parse_args()
    if args.leg:
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
        import torch
        assert torch.cuda.is_available(), 'needs the GPU'
        import crfconv_amd
        assert os.path.dirname(os.path.dirname(os.path.abspath(crfconv_amd.__file__))) == (os.path.abspath(args.tree) if args.tree else HERE)
        if args.leg == 'bits':
            np.savez(args.file, **leg_bits('cuda:0'))
        else:
            with open(args.file, 'w') as f:
                json.dump(leg_timing('cuda:0'), f)
        return
    if not args.parent:
        raise SystemExit('needs --parent DIR')
    os.makedirs(args.out_dir, exist_ok=True)
    lines = ['command: python scratch/transforms_refactor_ab.py --what %s --parent <parent checkout>' % args.what, '']

    def flush():
        text = '\n'.join(lines)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text + '\n')
        return text
    sides = (('parent', args.parent), ('new', None))
    if args.what in ('all', 'bits'):
        for name, tree in sides:
            child('bits', tree, os.path.join(args.out_dir, 'bits_%s.npz' % name), 600)
        a, b = (np.load(os.path.join(args.out_dir, 'bits_%s.npz' % name)) for name, _ in sides)
        same = [k for k in a.files if k in b.files and a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])]
        differ = sorted((set(a.files) | set(b.files)) - set(same))
        lines.append('(bits) tensors written by the parent %d, by the new tree %d, identical %d' % (len(a.files), len(b.files), len(same)))
        groups = {}
        for k in a.files:
            groups[k.split('/')[0]] = groups.get(k.split('/')[0], 0) + 1
        lines += ['    %-28s %d tensors' % (g, n) for g, n in sorted(groups.items())]
        lines += ['    DIFFERENT: %s' % k for k in differ] + ['']
        flush()
    if args.what in ('all', 'timing'):
        runs = []
        for i, (name, tree) in enumerate(sides * 2):
            path = os.path.join(args.out_dir, 'timing_%d_%s.json' % (i, name))
            child('timing', tree, path, 600)
            with open(path) as f:
                runs.append((name, json.load(f)))
        lines.append('(timing) per call, fresh processes in this order: %s.  Windows of each run; the new medians against the span of all '
                     'the parent\'s windows' % ' '.join(n for n, _ in runs))
        for key in runs[0][1]:
            lines.append('    %s' % key)
            for name, r in runs:
                lines.append('        %-6s %s   median %.2f' % (name, ' '.join('%.2f' % v for v in r[key]), float(np.median(r[key]))))
            span = [v for name, r in runs if name == 'parent' for v in r[key]]
            med = [float(np.median(r[key])) for name, r in runs if name == 'new']
            lines.append('        parent span [%.2f, %.2f]; new medians %s: %s' % (min(span), max(span), ' '.join('%.2f' % m for m in med),
                                                                                 'inside' if all(min(span) <= m <= max(span) for m in med)
                                                                                 else ('BELOW' if all(m <= max(span) for m in med) else 'ABOVE')))
        lines.append('')
        flush()
    if args.what in ('all', 'bench'):
        runs = []
        for name, tree in sides * 2:
            cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '100', '--warmup', '10']
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, cwd=os.path.abspath(tree) if tree else HERE)
            if p.returncode != 0:
                raise SystemExit('%s in %s failed with status %d: nothing further is started' % (' '.join(cmd), tree or HERE, p.returncode))
            runs.append((name, json.loads(p.stdout.strip().splitlines()[-1])))
            print('bench %s %s' % (name, runs[-1][1]), flush=True)
        lines.append('(bench) bench.py --gpus 1 --steps 100 --warmup 10, fresh processes in this order: %s' % ' '.join(n for n, _ in runs))
        for name in ('parent', 'new'):
            mine = [b for n, b in runs if n == name]
            lines.append('    %-6s ms_per_step %s   final_loss %s' % (name, ' '.join('%.4f' % b['ms_per_step'] for b in mine),
                                                                     ' '.join(repr(b['final_loss']) for b in mine)))
        lines += ['    final_loss equal in all four runs: %s' % (len({b['final_loss'] for _, b in runs}) == 1), '']
    print(flush())


if __name__ == '__main__':
    main()
