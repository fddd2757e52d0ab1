"""What the sliding block split on the device (crfconv_amd/blocks.py, csrc/blocks.hip) costs, against the reference's per-block loop.
profiles/r33_sliding_blocks.md holds what this prints.

    python scratch/sliding_blocks_timing.py --what all [--out FILE.md]        # every leg as a fresh process, the three ways alternating, twice
    python scratch/sliding_blocks_timing.py --what op|torch|numpy --shape npm3d|scannet        # one leg, one JSON line

Shapes:  npm3d    one scene of 2^20 points in about 60 x 45 x 8 m at the NPM3D parameters
         scannet  16 scenes of 65 536 points in about 8 x 6 x 3 m at the ScanNet parameters
Ways:    op       blocks.sliding_blocks (the whole call, its one host read included), and its two library calls apart
         torch    the reference's loop with boolean masks on the device: per scene min / max, per block one mask over the scene and the
                  two sum() reads the reference makes, then pos[cond], mask, indices
         numpy    the same loop on the host (the reference itself)
Device times are between two device events around `calls` back-to-back calls, after warm-up calls; the NumPy loop is on the host clock.
The op's algorithmic bytes: the positions are read by four launches (bounds, count, recount, emit: 4 x 12 N), the per-point row counts are
written and their scan read (8 N), the pairs are written (12 R), every sort pass moves 32 R, and the last launch reads the pairs (12 R) and
writes rows, indices, batch and mask (25 R)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {'npm3d': dict(scenes=1, n=1 << 20, box=(60.0, 45.0, 8.0), params='NPM3D'),
          'scannet': dict(scenes=16, n=65536, box=(8.0, 6.0, 3.0), params='SCANNET')}


def make(shape):
    sh = SHAPES[shape]
    rng = np.random.default_rng(3300)
    parts = [(rng.random((sh['n'], 3)) * np.asarray(sh['box']) + 10.0 * s).astype(np.float32) for s in range(sh['scenes'])]
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts), ptr


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
    import ctypes
    import torch
    from crfconv_amd import _lib, blocks
    from crfconv_amd.graph import ptr as p_, stream_ptr
    pos_h, ptr_h = make(shape)
    prm = getattr(blocks, SHAPES[shape]['params'])
    pos, ptr = torch.from_numpy(pos_h).cuda(), torch.from_numpy(ptr_h).cuda()
    split = blocks.sliding_blocks(pos, ptr, **prm)
    N, S, R, B = len(pos_h), len(ptr_h) - 1, split.n_rows, split.n_blocks
    out = {'n_blocks': B, 'n_rows': R, 'whole_ms': event_ms(lambda: blocks.sliding_blocks(pos, ptr, **prm), 10)}
    # the two library calls apart, on buffers made once
    spec = _lib.SlidingBlocksSpec(prm['block_size'], prm['stride'], prm['padding'], prm['proportion'], prm['min_points'],
                                  blocks.COUNT_FORMS[prm['count_form']])
    cap = blocks.CELL_CAP
    nbytes = _lib.call('crfconv_sliding_blocks_workspace', N, S, cap)
    ebytes = _lib.call('crfconv_sliding_blocks_emit_workspace', N, R)
    ws, ews = torch.empty(nbytes, dtype=torch.uint8, device='cuda'), torch.empty(ebytes, dtype=torch.uint8, device='cuda')
    totals = torch.empty(4, dtype=torch.int64, device='cuda')
    pos_min, limit = torch.empty_like(split.pos_min), torch.empty_like(split.limit)
    o = {k: torch.empty_like(getattr(split, k)) for k in ('ptr', 'rows', 'indices', 'mask', 'batch', 'scene', 'cell')}

    def count():
        _lib.call('crfconv_sliding_blocks_count', p_(pos), N, p_(ptr), S, ctypes.byref(spec), cap, p_(pos_min), p_(limit), p_(totals), p_(ws),
                  nbytes, stream_ptr())

    def emit():
        _lib.call('crfconv_sliding_blocks_emit', p_(pos), N, p_(ptr), S, ctypes.byref(spec), cap, p_(pos_min), B, R, p_(ws), nbytes, p_(ews),
                  ebytes, p_(o['ptr']), p_(o['rows']), p_(o['indices']), p_(o['mask']), p_(o['batch']), p_(o['scene']), p_(o['cell']), stream_ptr())
    count()
    out['count_ms'] = event_ms(count, 20)
    out['emit_ms'] = event_ms(emit, 20)
    assert all(torch.equal(o[k], getattr(split, k)) for k in o)
    extra = torch.rand((N, 3), device='cuda')
    out['features_room_ms'] = event_ms(lambda: split.features('room', extra), 20)
    out['features_block_ms'] = event_ms(lambda: split.features('block', extra), 20)
    passes = max(1, -(-max(B - 1, 1).bit_length() // 8))
    out['algorithmic_bytes'] = 4 * 12 * N + 2 * 4 * N + 12 * R + passes * 32 * R + 12 * R + 25 * R
    out['sort_passes'] = passes
    return out


def torch_loop(pos, ptr_h, prm):
    """The reference's loop, torch on the device: [(pos, mask, indices)] of the kept blocks."""
    import math
    import torch
    bs, st, pad = prm['block_size'], prm['stride'], prm['padding']
    kept = []
    for s in range(len(ptr_h) - 1):
        xyz = pos[ptr_h[s]:ptr_h[s + 1]]
        xyz = xyz - xyz.min(0).values
        limit = xyz.max(0).values.tolist()
        if prm['count_form'] == 'ratio':
            nx, ny = (int(math.ceil((v - bs) / st)) + 1 for v in limit[:2])
        else:
            nx, ny = (int(math.ceil(v - bs) / st) + 1 for v in limit[:2])
        idx = torch.arange(len(xyz), device=pos.device)
        for i in range(nx):
            for j in range(ny):
                xbeg, ybeg = i * st, j * st
                cond = (xyz[:, 0] >= xbeg - pad) & (xyz[:, 0] <= xbeg + bs + pad) & (xyz[:, 1] >= ybeg - pad) & (xyz[:, 1] <= ybeg + bs + pad)
                if int(cond.sum()) < prm['min_points']:
                    continue
                b = xyz[cond]
                mask = (b[:, 0] >= xbeg) & (b[:, 0] <= xbeg + bs) & (b[:, 1] >= ybeg) & (b[:, 1] <= ybeg + bs)
                if int(mask.sum()) / mask.shape[0] < prm['proportion']:
                    continue
                kept.append((b, mask.to(torch.int8), idx[cond]))
    return kept


def leg_torch(shape):
    import torch
    from crfconv_amd import blocks
    pos_h, ptr_h = make(shape)
    prm = getattr(blocks, SHAPES[shape]['params'])
    pos = torch.from_numpy(pos_h).cuda()
    kept = torch_loop(pos, ptr_h.tolist(), prm)
    return {'n_blocks': len(kept), 'n_rows': int(sum(len(k[0]) for k in kept)), 'whole_ms': event_ms(lambda: torch_loop(pos, ptr_h.tolist(), prm), 2, times=3, warm=1)}


def leg_numpy(shape):
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    sys.path.insert(0, os.path.join(HERE, 'tests', 'golden'))
    import sliding_blocks_restatement as R
    pos_h, ptr_h = make(shape)
    prm = getattr(R, SHAPES[shape]['params'])
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        split = R.np_sliding_blocks(pos_h, ptr_h, **prm)
        ms.append((time.perf_counter() - t) * 1e3)
    return {'n_blocks': split['n_blocks'], 'n_rows': int(split['n_rows']), 'whole_ms': ms}


LEGS = {'op': leg_op, 'torch': leg_torch, 'numpy': leg_numpy}


def run_leg(what, shape):
    cmd = [sys.executable, os.path.abspath(__file__), '--what', what, '--shape', shape]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d: nothing further is started' % (' '.join(cmd), p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['all'] + sorted(LEGS))
    ap.add_argument('--shape', default='npm3d', choices=sorted(SHAPES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.what != 'all':
        print(json.dumps(LEGS[args.what](args.shape)))
        return
    lines = ['command: python scratch/sliding_blocks_timing.py --what all; ms per call, median (minimum); fresh processes, the three ways alternating, twice', '']
    for shape in ('npm3d', 'scannet'):
        runs = [(what, run_leg(what, shape)) for what in ('op', 'torch', 'numpy') * 2]
        lines.append('%s: %d scene(s) x %d points' % (shape, SHAPES[shape]['scenes'], SHAPES[shape]['n']))
        for what in ('op', 'torch', 'numpy'):
            mine = [r for w, r in runs if w == what]
            lines.append('    %-6s blocks %d rows %d   whole %s' % (what, mine[0]['n_blocks'], mine[0]['n_rows'],
                                                                 '   '.join('%.3f (%.3f)' % (np.median(r['whole_ms']), min(r['whole_ms'])) for r in mine)))
        for r in (r for w, r in runs if w == 'op'):
            dev_ms = float(np.median(r['count_ms']) + np.median(r['emit_ms']))
            lines.append('    op     count %.3f   emit %.3f   features room %.3f block %.3f   sort passes %d   %.1f MB algorithmic -> %.0f GB/s over '
                         'count + emit (%.1f %% of 8 TB/s)' % (np.median(r['count_ms']), np.median(r['emit_ms']), np.median(r['features_room_ms']),
                                                               np.median(r['features_block_ms']), r['sort_passes'], r['algorithmic_bytes'] / 1e6,
                                                               r['algorithmic_bytes'] / dev_ms / 1e6, r['algorithmic_bytes'] / dev_ms / 1e6 / 80.0))
        lines.append('    blocks and rows equal in all runs: %s' % (len({(r['n_blocks'], r['n_rows']) for _, r in runs}) == 1))
        lines.append('')
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
