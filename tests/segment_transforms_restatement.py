"""The ragged-batch transform chain of crfconv_amd.transforms.SegmentCompose (csrc/augment_segments.hip) restated in numpy float64
from ptr, params [S, 8], stats [S, 4], the noise and the picks.  No GPU code: tests/test_host_segment_transforms.py checks this
module against a plain float64 torch composition, tests/test_gpu_segment_transforms.py checks the kernels against it.

Per cloud b (rows ptr[b] .. ptr[b + 1]), every step optional, in this order:
    center     p <- p - c                         c = stats[b, 0:3]
    normalize  p <- p * k                         k = stats[b, 3]
    rotate     p <- p @ M                         x_a' = c x_a - s x_b, x_b' = s x_a + c x_b, (a, b) = (axis + 1, axis + 2) mod 3,
                                                  (c, s) = params[b, 0:2]
    scale      p <- p * s                         s = params[b, 2:5]
    flip       p_i <- max(p_i) - p_i              for the axes in params[b, 5] & flip_axes; the max over the cloud at this point
    noise      p <- p + clamp(noise, -clip, clip)
    normals    n <- n @ M;  n <- n / s, then n / |n| (a zero normal stays zero) when the chain scales;  n_i <- -n_i on a flipped axis
    x          [p] (C = 3), [p, n] (x_norm) or [p, rgb], rgb <- 0 where params[b, 6] == 0 and the chain drops
"""
import numpy as np


def gather(index, *arrays):
    """FixedPoints' effect on row attributes: each array indexed by the picks (GLOBAL rows)."""
    return [None if a is None else np.asarray(a)[np.asarray(index)] for a in arrays]


def restate(pos, ptr, params, stats, *, norm=None, rgb=None, noise=None, center=False, normalize=False, axis=None, scale=False,
            flip_axes=0, clip=None, drop=False, x_layout=None):
    """Returns dict(pos [N, 3], norm [N, 3] or None, x [N, C] or None, R [S], Rn [S], cmax [S, 3]): float64; R[b] is the largest
    magnitude of any value COMPUTED for a position of cloud b along the chain (the input itself is not one), Rn[b] the same for its
    normals (0 without), cmax[b, i] the maximum the flip of axis i subtracts from (0 when not flipped)."""
    p_all = np.array(pos, dtype=np.float64)
    n_all = None if norm is None else np.array(norm, dtype=np.float64)
    c_all = None if rgb is None else np.array(rgb, dtype=np.float64)
    ptr = np.asarray(ptr, dtype=np.int64)
    params, stats = np.asarray(params, dtype=np.float64), np.asarray(stats, dtype=np.float64)
    S = len(ptr) - 1
    R, Rn, cmax = np.zeros(S), np.zeros(S), np.zeros((S, 3))

    def rot(v, b):
        c, s = params[b, 0], params[b, 1]
        ia, ib = (axis + 1) % 3, (axis + 2) % 3
        xa, xb = v[:, ia].copy(), v[:, ib].copy()
        parts = [c * xa, s * xb, s * xa, c * xb]
        v[:, ia], v[:, ib] = parts[0] - parts[1], parts[2] + parts[3]
        return max([0.0] + [float(np.abs(q).max()) for q in parts if q.size])

    for b in range(S):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        if hi <= lo:
            continue
        p = p_all[lo:hi]
        seen = [0.0]

        def see(v):
            seen.append(float(np.abs(v).max()))
        if center:
            p -= stats[b, 0:3]
            see(p)
        if normalize:
            p *= stats[b, 3]
            see(p)
        if axis is not None:
            seen.append(rot(p, b))
            see(p)
        if scale:
            p *= params[b, 2:5]
            see(p)
        flip = int(params[b, 5]) & flip_axes
        for i in range(3):
            if (flip >> i) & 1:
                cmax[b, i] = p[:, i].max()
                p[:, i] = cmax[b, i] - p[:, i]
        see(p)
        if noise is not None:
            p += np.clip(np.asarray(noise, dtype=np.float64)[lo:hi], -clip, clip)
            see(p)
        R[b] = max(seen)
        if n_all is not None:
            n = n_all[lo:hi]
            seen = [0.0]
            if axis is not None:
                seen.append(rot(n, b))
                see(n)
            if scale:
                n /= params[b, 2:5]
                see(n)
                length = np.sqrt((n * n).sum(1, keepdims=True))
                np.divide(n, length, out=n, where=length > 0)
            for i in range(3):
                if (flip >> i) & 1:
                    n[:, i] = -n[:, i]
            see(n)
            Rn[b] = max(seen)
        if c_all is not None and drop and params[b, 6] == 0:
            c_all[lo:hi] = 0
    x = None
    if x_layout == 'pos':
        x = p_all.copy()
    elif x_layout == 'pos_norm':
        x = np.concatenate([p_all, n_all], 1)
    elif x_layout == 'pos_rgb':
        x = np.concatenate([p_all, c_all], 1)
    return {'pos': p_all, 'norm': n_all, 'x': x, 'R': R, 'Rn': Rn, 'cmax': cmax}
