"""-m gpu: ops.crf_meanfield, form by form, against float64 references written here in plain torch with autograd on the CPU -- the fused
first step, the fast and the generic steps of csrc/crf.hip, the restructured backward of csrc/crf_bwd.hip (reverse walks, the edge pass
over all steps, the in-launch dP / dQ slab reduction at H = 8 / 16), the per-step backward of csrc/crf_step_bwd.hip, the block-resident
forward of csrc/crf_block.hip, the one-point-per-wavefront kernels of csrc/crf_wide.hip and csrc/crf_matrices.hip.

The reference restates  x_0 = z,  x_t = z Q + (A x_{t-1}) P,  A = row-softmax(-|y_i - y_j|^2) over the valid entries of columns k0 .. K-1,
a row without a valid entry sending no message; it is driven by the table AS THE DEVICE HOLDS IT (tab.idx32 read back, < 0 = no
neighbour) and has two entry forms: from c (Q = (I + c^T c)^-1, P = c^T c Q: gives dc) and from leaf Q, P (gives dQ and dP SEPARATELY --
with P = I - Q, dc sees gQ - gP alone and an error that lands equally in both cancels there).  Each runs once in float64, once in float32.

The comparison is test_gpu_discrete's `own_scale` on every tensor's OWN scale: e = max|got - ref64| / max|ref64| <= max(bound, 4 e32), and
e32 <= bound is asserted too, so the second branch never decides.  A bound belongs to a SITE (group of cases x tensor, BOUNDS below) and
is ~10 x the largest e32 the float32 restatement showed on the CPU over that site's cases (the factor: another summation order); inputs
are scaled for it (y by 1.5 / sqrt(H): distances of order 1; z and gout with a mean away from 0, so that the H x H gradients are sums
that do not cancel; the reference multiplies in 64-row blocks, `rows_matmul`, so that its float32 run does not depend on a BLAS's
summation order).  A reference tensor that is structurally zero (dy at T = 0, dP without an edge ...) asks for exact zeros; the two
tensors that are zero by cancellation only (dc of a graph of self-loops, dy of equal y rows) are judged on the scale of the terms they
cancel from (`judge`).  Before every backward the
allocator is poisoned with NaN blocks of each gradient's shape, every output is asserted finite, and for every case the rule must refuse
each tensor zeroed and mis-scaled by 10 x its bound (arithmetic on results already computed, no launch).

The kernels' geometry (Geo, Scat, Rev, RS_CHUNKS) is READ from csrc/crf_common.hpp and csrc/crf_bwd.hip: the macro defaults and constants
by name, the formulas restated beside them (`geometry`).  Measured figures per site: BOUNDS and profiles/r26_meanfield_float64.md."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import DEV, t
from test_gpu_discrete import dev, device_rows, edges_table, f32, index_table, leaf, own_scale, poison, rejected, shaped_rows

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crfconv_amd', 'csrc')
NARROW = (4, 8, 16, 32, 64)

# site -> tensor -> (bound, largest e32 of the float32 restatement on the CPU, largest e measured on the MI355X); bound ~ 10 x e32.
# A site is one group of cases (the test named beside it) in one width family.
BOUNDS = {
    'fast':     dict(out=(7e-06, 6.3e-07, 7.3e-07), dz=(6e-06, 5.1e-07, 6.2e-07), dy=(1e-05, 9.6e-07, 1.3e-06),
                     dc=(5e-05, 5.0e-06, 7.4e-07), dQ=(3e-06, 2.1e-07, 1.2e-07), dP=(3e-06, 2.2e-07, 1.9e-07)),
    'rows':     dict(out=(1e-05, 9.2e-07, 6.5e-07), dz=(7e-06, 6.4e-07, 5.5e-07), dy=(1e-05, 9.8e-07, 1.1e-06),
                     dc=(4e-05, 3.1e-06, 7.0e-07), dQ=(4e-06, 3.1e-07, 1.5e-07), dP=(4e-06, 3.5e-07, 4.2e-07)),
    'slab':     dict(out=(3e-06, 2.2e-07, 3.3e-07), dz=(4e-06, 3.8e-07, 3.8e-07), dy=(4e-06, 3.2e-07, 3.1e-07),
                     dQ=(2e-06, 1.8e-07, 3.3e-07), dP=(2e-06, 1.6e-07, 4.4e-07)),
    'indeg':    dict(out=(6e-06, 5.9e-07, 6.5e-07), dz=(2e-05, 1.9e-06, 8.1e-07), dy=(2e-05, 1.8e-06, 2.1e-06),
                     dc=(4e-05, 3.2e-06, 5.0e-07), dQ=(3e-06, 2.3e-07, 1.3e-07), dP=(2e-06, 1.8e-07, 1.6e-07)),
    'generic':  dict(out=(2e-05, 1.1e-06, 9.9e-07), dz=(2e-05, 1.1e-06, 5.6e-07), dy=(2e-05, 1.4e-06, 1.3e-06),
                     dc=(7e-05, 6.2e-06, 9.5e-07), dQ=(3e-06, 2.9e-07, 1.6e-07), dP=(3e-06, 2.7e-07, 2.1e-07)),
    'wide':     dict(out=(2e-05, 1.3e-06, 1.2e-06), dz=(2e-05, 1.3e-06, 1.2e-06), dy=(2e-05, 1.5e-06, 1.7e-06),
                     dc=(8e-05, 7.8e-06, 1.5e-06), dQ=(4e-06, 3.1e-07, 1.7e-07), dP=(4e-06, 3.3e-07, 3.1e-07)),
    'padded':   dict(out=(7e-06, 7.0e-07, 7.3e-07), dz=(8e-06, 7.8e-07, 5.8e-07), dy=(1e-05, 9.9e-07, 6.5e-07),
                     dc=(4e-05, 4.0e-06, 5.6e-07), dQ=(3e-06, 2.8e-07, 1.2e-07), dP=(3e-06, 2.1e-07, 2.0e-07)),
    'regime':   dict(out=(1e-05, 9.2e-07, 8.7e-07), dz=(9e-06, 8.3e-07, 1.0e-06), dy=(2e-05, 1.1e-06, 1.3e-06),
                     dc=(8e-05, 7.3e-06, 1.5e-06), dQ=(2e-06, 2.0e-07, 1.6e-07), dP=(3e-06, 2.7e-07, 2.3e-07)),
    'regime_g': dict(out=(8e-06, 7.7e-07, 8.8e-07), dz=(1e-05, 9.4e-07, 6.2e-07), dy=(1e-05, 1.0e-06, 7.5e-07),
                     dc=(4e-04, 3.6e-05, 4.6e-06), dQ=(3e-06, 2.6e-07, 2.1e-07), dP=(2e-06, 2.0e-07, 1.8e-07)),
    'forms':    dict(out=(7e-06, 6.6e-07, 6.0e-07), dz=(6e-06, 5.7e-07, 4.9e-07), dy=(9e-06, 8.5e-07, 6.1e-07),
                     dc=(4e-05, 4.0e-06, 6.2e-07), dQ=(2e-06, 1.7e-07, 1.2e-07), dP=(3e-06, 2.1e-07, 2.0e-07)),
}


def bound(site, name):
    return BOUNDS[site][name][0]


# ------------------------------------------------------------------ the kernels' geometry, read from the sources
def _csrc_int(fname, name):
    """The integer a source file gives `name`: `#define name N` (the default under #ifndef) or `constexpr int name = N;`."""
    text = open(os.path.join(CSRC, fname)).read()
    hit = re.search(r'#define\s+%s\s+(\d+)' % name, text) or re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert hit, '%s: no %s' % (fname, name)
    return int(hit.group(1))


def geometry(H):
    """Rows per wavefront / workgroup of the mean-field kernels at width H, the formulas of the sources restated:
    Geo<H>: L = H / 4, PPW = WAVE / L, PPB = PPW * (BLOCK / WAVE)                                      (crf_common.hpp)
    Scat<H>: EP = L <= 4 ? SCAT_EP : 1, RPW = WAVE / (L EP), RPB = RPW * (BLOCK / WAVE)                (crf_common.hpp)
    Rev<H, EPV>: NW = H >= 32 ? 1 : BLOCK / WAVE, R = WAVE / (L EPV), RPB = R NW, CAP = 64 * ((R * 16 * REV_HEAD / 100 + 63) / 64), with
    EPV of the chain and of the final walk as launch_rev chooses them                                    (crf_bwd.hip)."""
    wave = 64
    block = _csrc_int('crf_common.hpp', 'BLOCK')
    L = H // 4
    g = dict(PPW=wave // L, PPB=wave // L * (block // wave))
    ep = _csrc_int('crf_common.hpp', 'SCAT_EP') if L <= 4 else 1
    g['SCAT_RPW'], g['SCAT_RPB'] = wave // (L * ep), wave // (L * ep) * (block // wave)
    head = _csrc_int('crf_bwd.hip', 'REV_HEAD')
    chain = 4 if H == 4 else (_csrc_int('crf_bwd.hip', 'REV_EP_CHAIN') if H <= 8 else _csrc_int('crf_bwd.hip', 'REV_EP_CHAIN16'))
    final = 4 if H == 4 else (_csrc_int('crf_bwd.hip', 'REV_EP_FINAL16') if H == 16 else
                              _csrc_int('crf_bwd.hip', 'REV_EP_FINAL') if H <= 8 else _csrc_int('crf_bwd.hip', 'REV_EP_CHAIN16'))
    g['REV'] = []
    for epv in sorted({chain, final}):
        R = wave // (L * epv)
        g['REV'].append(dict(R=R, RPB=R * (1 if H >= 32 else block // wave), CAP=64 * ((R * 16 * head // 100 + 63) // 64)))
    g['RS_CHUNKS'] = _csrc_int('crf_common.hpp', 'RS_CHUNKS')
    return g


# ------------------------------------------------------------------ float64 / float32 reference (plain torch, autograd)
def ref_weights(y, rows, k0, keep=None):
    """A [m, K]: row-softmax of -|y_i - y_j|^2 over the valid entries of columns k0 .., 0 elsewhere; a row without one is all 0.
    keep: a list that receives A with its gradient retained."""
    m, K = rows.shape
    H = y.shape[1]
    valid = rows >= 0
    valid[:, :k0] = False
    j = rows.clamp(min=0)
    step = max(1, int(2e7 // (K * H)))
    d = torch.cat([((y[j[lo:lo + step]] - y[lo:lo + step, None, :]) ** 2).sum(-1) for lo in range(0, m, step)])
    big = torch.finfo(y.dtype).max
    dmin = torch.where(valid, d, torch.full((), big, dtype=y.dtype)).min(1).values.detach()
    dmin = torch.where(valid.any(1), dmin, torch.zeros((), dtype=y.dtype))
    w = torch.where(valid, torch.exp(torch.where(valid, dmin[:, None] - d, torch.zeros((), dtype=y.dtype))), torch.zeros((), dtype=y.dtype))
    A = w / w.sum(1, keepdim=True).clamp(min=torch.finfo(y.dtype).tiny)
    if keep is not None and A.requires_grad:
        A.retain_grad()
        keep.append(A)
    return A, valid


def rows_matmul(x, M, blk=64):
    """x M for x [m, H], as a batch of 64-row blocks against the expanded M: the gradient of M is then a sum of per-block products over the
    block axis (torch.sum: a cascade), not one product with inner dimension m whose float32 summation order is the BLAS's own -- the
    float32 restatement's dQ at 32 771 rows was 1.8e-7 from float64 on one CPU and 2.5e-6 on another before this."""
    m, H = x.shape
    n = -(-m // blk)
    xp = torch.nn.functional.pad(x, (0, 0, 0, n * blk - m)) if n * blk != m else x
    return torch.bmm(xp.view(n, blk, H), M.expand(n, H, H)).reshape(n * blk, H)[:m]


def ref_meanfield(z, y, Q, P, rows, k0, T, keep=None):
    m, K = rows.shape
    H = z.shape[1]
    A, _ = ref_weights(y, rows, k0, keep)
    j = rows.clamp(min=0)
    step = max(1, int(2e7 // (K * H)))
    x = z
    zq = rows_matmul(z, Q)
    for _ in range(T):
        msg = torch.cat([(A[lo:lo + step, :, None] * x[j[lo:lo + step]]).sum(1) for lo in range(0, m, step)])
        x = zq + rows_matmul(msg, P)
    return x


def matrices(c):
    M = c.t() @ c
    Q = torch.linalg.inv(torch.eye(c.shape[0], dtype=c.dtype) + M)
    return Q, M @ Q


def mf_reference(z, y, c, rows, k0, T, gout, dtype, QP=None):
    """{out, dz, dy, dc} from c, or {out, dz, dy, dQ, dP} from the given (Q, P); a gradient nothing reaches is a zero tensor."""
    zl, yl = leaf(z, dtype), leaf(y, dtype)
    if QP is None:
        mats = [leaf(c, dtype)]
        Q, P = matrices(mats[0])
        names = ('dc',)
    else:
        mats = [leaf(QP[0], dtype), leaf(QP[1], dtype)]
        Q, P = mats
        names = ('dQ', 'dP')
    keep = []
    x = ref_meanfield(zl, yl, Q, P, rows, k0, T, keep)
    (x * gout.to(dtype)).sum().backward()
    res = dict(out=x.detach().clone())
    for k, v in zip(('dz', 'dy') + names, [zl, yl] + mats):
        res[k] = torch.zeros_like(v) if v.grad is None else v.grad
    # the scale of the terms dy is summed from: dy_i = sum_k w_ik (y_i - y_j) + sum_{e = (t, k) -> i} w_e (y_i - y_t) with
    # w_ik = -2 A_ik (gA_ik - <A_i, gA_i>), gA = dL / dA: |w_ik| <= 4 A_ik max_k |gA_ik|
    if T == 0 or not keep or keep[0].grad is None:
        gd = torch.zeros(rows.shape, dtype=dtype)
    else:
        gd = 4.0 * keep[0].detach() * keep[0].grad.abs().max(1, keepdim=True).values
    into = torch.zeros(rows.shape[0], dtype=dtype).index_add_(0, rows.clamp(min=0).reshape(-1), gd.reshape(-1))      # (A is 0 where no entry)
    res['_dy_terms'] = float(y.abs().max()) * float((gd.sum(1) + into).max())
    return res


def mf_run(z, y, c, tab, k0, T, gout, QP=None, need='zym'):
    """ops.crf_meanfield forward + backward on host tensors as given (a strided z / y / gout goes in as it is): from c, or from leaf
    (Q, P) through matrices= (H <= 64) and through _MeanFieldWide with the channels padded as crf_meanfield pads them (H > 64).
    need: which of z, y and the matrices (c or Q, P) require grad."""
    from crfconv_amd import ops
    from crfconv_amd.ops.crf import _MeanFieldWide
    m, H = z.shape
    zd, yd = dev(z).requires_grad_('z' in need), dev(y).requires_grad_('y' in need)
    if z.stride() != z.contiguous().stride():                       # a column slice of a wider device tensor, like the host one
        wide = torch.zeros(m, 2 * H + 3, device=DEV)
        wide[:, 1:2 * H + 1:2] = dev(z)
        zd = wide[:, 1:2 * H + 1:2].detach().requires_grad_('z' in need)
        wide = torch.zeros(m, 2 * H + 3, device=DEV)
        wide[:, 2:2 * H + 2:2] = dev(y)
        yd = wide[:, 2:2 * H + 2:2].detach().requires_grad_('y' in need)
        assert not zd.is_contiguous() and not yd.is_contiguous()
    poison((m, H), (T, m, H))
    if QP is None:
        mats = [dev(c).requires_grad_('m' in need)]
        out = ops.crf_meanfield(zd, yd, mats[0], tab, T, k0=k0)
        names = ('dc',)
    else:
        mats = [dev(QP[0]).requires_grad_('m' in need), dev(QP[1]).requires_grad_('m' in need)]
        names = ('dQ', 'dP')
        if H <= 64:
            out = ops.crf_meanfield(zd, yd, None, tab, T, k0=k0, matrices=tuple(mats))
        else:
            Hp = 128 if H <= 128 else 256
            pad = torch.nn.functional.pad
            out = _MeanFieldWide.apply(pad(zd, (0, Hp - H)), pad(yd, (0, Hp - H)), pad(mats[0], (0, Hp - H, 0, Hp - H)),
                                       pad(mats[1], (0, Hp - H, 0, Hp - H)), tab, k0, T)[:, :H]
    assert out.shape == (m, H)
    Hp = H if H > 64 else [w for w in NARROW if w >= H][0]
    poison((m, Hp), (m, Hp), (m, Hp), (m, tab.K), (T, m, Hp), (T, m, Hp), (Hp, Hp), (Hp, Hp), (m, Hp), (m, Hp))
    if gout.stride() == gout.contiguous().stride():
        gd = dev(gout)
    elif 0 in gout.stride():                                        # an expanded gradient: stride 0 on the device too
        gd = dev(gout[:1]).expand(m, H)
    else:
        wide = torch.zeros(m, 2 * H + 1, device=DEV)
        wide[:, 0:2 * H:2] = dev(gout)
        gd = wide[:, 0:2 * H:2]
    out.backward(gd)
    res = dict(out=out.detach().cpu())
    for k, v, flag in zip(('dz', 'dy') + names, [zd, yd] + mats, ('z', 'y') + ('m',) * len(mats)):
        assert (v.grad is not None) == (flag in need), k
        if v.grad is not None:
            assert tuple(v.grad.shape) == tuple(v.shape), k
            res[k] = v.grad.cpu()
    return res


def judge(site, got, r32, r64, cancelled=None):
    """Every tensor of `got` against float64 on its own scale within the site's bound; exact zeros where the reference is structurally
    zero; and the rule refuses each tensor zeroed and mis-scaled by 10 x its bound.
    cancelled = {name: scale}: a tensor that is zero in exact arithmetic without being structurally zero (dc of a graph of self-loops:
    x_t = z (Q + P) = z, so gQ = gP and dc = -c (S + S^T), S = Q (gQ - gP) Q, cancels to rounding) has no scale of its own; its distance
    from the float64 result is measured on the scale given (that of the gQ it cancels from), under the same rule.  dy where all y rows are
    equal is the other such tensor (below)."""
    cancelled = dict(cancelled or {})
    if float(r64['dy'].abs().max()) == 0.0 and r64['_dy_terms'] > 0.0:
        # every difference y_i - y_j is 0 (one row, identical rows) while gradients do reach the distances: dy is a sum of terms that
        # cancel, zero to rounding in whatever order a kernel adds them (the final walk forms (sum w) y_i - sum w y_t), not structurally
        cancelled['dy'] = r64['_dy_terms']
    for k in got:
        g = got[k].detach().cpu()
        assert tuple(g.shape) == tuple(r64[k].shape), k
        assert bool(torch.isfinite(g).all()), '%s.%s is not finite' % (site, k)
        if float(r64[k].abs().max()) == 0.0 and k not in cancelled:
            assert torch.equal(g, torch.zeros_like(g)), '%s.%s: the reference is structurally zero, the result is not' % (site, k)
            print('[own_scale] %-12s exact zeros' % (site + '.' + k), flush=True)
            continue
        b = bound(site, k)
        if cancelled and k in cancelled:
            e = float((g.double() - r64[k]).abs().max()) / cancelled[k]
            e32 = float((r32[k].double() - r64[k]).abs().max()) / cancelled[k]
            print('[own_scale] %-12s e %.3e  e32 %.3e  bound %.1e  (cancelled: on the scale of its terms)' % (site + '.' + k, e, e32, b), flush=True)
            assert e32 <= b and e <= max(b, 4.0 * e32), '%s.%s: %.3e of the scale it cancels from (e32 %.3e, bound %.1e)' % (site, k, e, e32, b)
            continue
        own_scale(g, r32[k], r64[k], b, site + '.' + k)
        assert rejected(torch.zeros_like(g), r32[k], r64[k], b), '%s.%s zeroed passes' % (site, k)
        assert rejected(g.double() * (1.0 + 10.0 * b), r32[k], r64[k], b), '%s.%s mis-scaled by 10 x the bound passes' % (site, k)


def mf_inputs(rng, m, H):
    """z in -0.5 .. 1 and gout = 0.3 + 0.5 N(0, 1) + 0.8 z (no direction of symmetry, means away from 0: dQ = z^T sum G and dP = sum m^T G
    are sums over all rows that do not cancel; the part along z keeps gQ - gP = sum (z - m_t)^T G_t, all that dc sees, from cancelling to
    1 / sqrt(rows) of its terms); y scaled so that |y_i - y_j|^2 is of order 1 at every H; c of spectral norm ~1."""
    z = f32(rng, (m, H), -0.5, 1.0)
    y = f32(rng, (m, H), -1.0, 1.0) * np.float32(1.5 / np.sqrt(H))
    c = torch.from_numpy((0.8 * rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32))
    gout = torch.from_numpy((0.3 + 0.5 * rng.standard_normal((m, H))).astype(np.float32)) + np.float32(0.8) * z
    return z, y, c, gout


def given_matrices(c):
    """(Q, P) of c as float32 leaves-to-be: computed in float64, rounded once (both references and the device read these values)."""
    Q, P = matrices(c.double())
    return Q.float(), P.float()


def mf_check(site, z, y, c, tab, k0, T, gout, forms=('QP', 'c')):
    """One case in both entry forms.  Returns {form: (got, r32, r64)}."""
    rows = device_rows(tab)
    m = z.shape[0]
    assert rows.shape[0] == m and int(rows.max()) < m
    used = rows[:, k0:]
    loops_only = T > 0 and bool(((used < 0) | (used == torch.arange(m)[:, None])).all()) and bool((used >= 0).any(1).all())
    seen = {}
    for form in forms:
        QP = given_matrices(c) if form == 'QP' else None
        r64 = mf_reference(z, y, c, rows, k0, T, gout, torch.float64, QP)
        r32 = mf_reference(z, y, c, rows, k0, T, gout, torch.float32, QP)
        got = mf_run(z, y, c, tab, k0, T, gout, QP)
        # every row averages over itself alone: dc cancels (judge), on the scale of the dQ of the same case
        judge(site, got, r32, r64, cancelled=dict(dc=float(seen['QP'][2]['dQ'].abs().max())) if loops_only and form == 'c' else None)
        seen[form] = (got, r32, r64)
    return seen


def dense_table(rows, n_src):
    """[B, n, K] per-cloud ids without holes -> NeighborTable (the device re-sorts columns 1..; uint16 ids beside int32 when K % 8 == 0)."""
    from crfconv_amd.graph import NeighborTable
    rows = np.asarray(rows)
    assert rows.ndim == 3 and rows.min() >= 0 and rows.max() < n_src
    return NeighborTable(t(rows.astype(np.int64)), n_src)


def knn_like(rng, B, n, K):
    """[B, n, K] per-cloud ids: column 0 the row itself (the column k0 = 1 drops), the others anywhere in the cloud."""
    rows = rng.integers(0, n, (B, n, K))
    rows[:, :, 0] = np.arange(n)[None]
    return rows


def without_idx16(tab):
    """The same table object with the uint16 ids dropped: every kernel takes its int32 index form (U16 = false)."""
    other = copy.copy(tab)
    other.idx16 = None
    other.cache = {}
    return other


def supported(H, K, k0):
    from crfconv_amd import _lib
    Hp = H if H > 64 else [w for w in NARROW if w >= H][0]
    return _lib.load().crfconv_meanfield_backward_supported(Hp, K, k0)


# ------------------------------------------------------------------ 1 + 2: fast forms, both index layouts
@pytest.mark.parametrize('K', [16, 32])
@pytest.mark.parametrize('H', NARROW)
def test_fast_forms_and_index_layouts(H, K):
    """Every (H, K) of the fast kernels (fused first step + step_fast_kernel<H, K>, bwd_edge_all_kernel<H, K>, the KSH = 4 / 5 reverse
    walks), k0 = 1, dense NeighborTable of B = 3 clouds of 67 rows (67 is prime: the uint16 decode row / n_tgt changes cloud inside a
    wavefront at every width), T = 3; at H = 8 and 64 also T = 0, 1, 2 and 5.  From c: out, dz, dy, dc; from leaf (Q, P): dQ and dP each.
    The same inputs through the same table without its uint16 ids (U16 = false in every kernel) must give the same bits for the forward
    and every gradient.  (H, K) = (8, 16) also runs with ops.state.mf_block = 'on': the block-resident forward of crf_block.hip.
    Bounds and CPU e32: BOUNDS['fast'].
    Largest e measured on the MI355X: out 7.3e-07, dz 6.2e-07, dy 1.3e-06, dc 7.4e-07, dQ 1.2e-07, dP 1.9e-07."""
    from crfconv_amd import _lib, ops
    B, n = 3, 67
    rng = np.random.default_rng(100 * H + K)
    tab = dense_table(knn_like(rng, B, n, K), n)
    assert not tab.padded and tab.idx16 is not None and supported(H, K, 1) == 1
    bare = without_idx16(tab)
    z, y, c, gout = mf_inputs(rng, B * n, H)
    for T in ((0, 1, 2, 3, 5) if H in (8, 64) else (3,)):
        seen = mf_check('fast', z, y, c, tab, 1, T, gout)
        for form, (got, _, _) in seen.items():
            other = mf_run(z, y, c, bare, 1, T, gout, given_matrices(c) if form == 'QP' else None)
            for k in got:
                assert torch.equal(other[k], got[k]), 'int32 index layout differs from uint16 in %s (T = %d, from %s)' % (k, T, form)
    if (H, K) == (8, 16):
        assert _lib.load().crfconv_meanfield_forward_block_rows(B * n, H, K, 1, 3) > 0
        ops.state.mf_block = 'on'
        try:
            mf_check('fast', z, y, c, tab, 1, 3, gout, forms=('c',))
        finally:
            ops.state.mf_block = 'auto'


# ------------------------------------------------------------------ 3: row counts around every rows-per-wave / rows-per-workgroup
@pytest.mark.parametrize('form', ['fast', 'generic'])
@pytest.mark.parametrize('H', NARROW)
def test_row_counts(H, form):
    """One cloud of m rows, m = 1 and one below / above Geo<H>::PPW and PPB, Scat<H>::RPW and RPB, Rev<H, EPV>::R and RPB of both walks, and
    3 PPB + PPW + 1: the lanes past m are aliased onto row m - 1 in every kernel, and here a double-counted alias is a large part of a
    sum.  m = 1: every neighbour is row 0.  fast: K = 16, k0 = 1, dense; generic: K = 9, k0 = 1, dense.  T = 2.
    Bounds and CPU e32: BOUNDS['rows'].
    Largest e measured on the MI355X: out 6.5e-07, dz 5.5e-07, dy 1.1e-06, dc 7.0e-07, dQ 1.5e-07, dP 4.2e-07."""
    g = geometry(H)
    marks = {g['PPW'], g['PPB'], g['SCAT_RPW'], g['SCAT_RPB']} | {r['R'] for r in g['REV']} | {r['RPB'] for r in g['REV']}
    ms = sorted({1, 3 * g['PPB'] + g['PPW'] + 1} | {v + d for v in marks for d in (-1, 1) if v + d >= 1})
    K = 16 if form == 'fast' else 9
    assert supported(H, K, 1) == (1 if form == 'fast' else 0)
    for m in ms:
        rng = np.random.default_rng(1000 * H + m)
        tab = dense_table(knn_like(rng, 1, m, K), m)
        z, y, c, gout = mf_inputs(rng, m, H)
        mf_check('rows', z, y, c, tab, 1, 2, gout)


# ------------------------------------------------------------------ 4: the slab reduction of dP / dQ at H = 8 / 16
@pytest.mark.parametrize('nblk', [127, 128, 129, 257])
@pytest.mark.parametrize('H', [8, 16])
def test_slab_reduction(H, nblk):
    """bwd_edge_all_kernel leaves one dP and one dQ slab per workgroup; reduce_small_body sums them in RS_CHUNKS = 128 chunks of
    per = ceil(nblk / 128) slabs.  nblk = 127: per = 1 and an empty chunk; 128: per = 1, every chunk full; 129: per = 2, chunks 65 .. 127
    empty and chunk 64 ragged; 257: per = 3, the last used chunk ragged.  m = (nblk - 1) PPB + 3: the last workgroup holds three rows.
    K = 16, k0 = 1, T = 2, one cloud.  dQ and dP directly, from leaf (Q, P).
    Bounds and CPU e32: BOUNDS['slab'].
    Largest e measured on the MI355X: out 3.3e-07, dz 3.8e-07, dy 3.1e-07, dQ 3.3e-07, dP 4.4e-07."""
    from crfconv_amd import _lib
    g = geometry(H)
    assert g['RS_CHUNKS'] == 128 and _lib.load().crfconv_meanfield_backward_param_grads_inside(H) == 1
    m = (nblk - 1) * g['PPB'] + 3
    assert -(-m // g['PPB']) == nblk and m * H <= 33000 * 8
    rng = np.random.default_rng(10 * nblk + H)
    tab = dense_table(knn_like(rng, 1, m, 16), m)
    z, y, c, gout = mf_inputs(rng, m, H)
    mf_check('slab', z, y, c, tab, 1, 2, gout, forms=('QP',))


# ------------------------------------------------------------------ 5: in-degrees of the reverse walks
def indegree_rows(rng, m, K, revs):
    """[1, m, K] whose in-degrees (all K columns: the reverse list holds column 0 too, with weight 0) follow a plan:
    hubs at rows 0, 5 and m - 1 (in-degree m - 1: odd); for every Rev geometry (R, CAP) four windows of R consecutive, R-aligned rows whose
    in-degrees total CAP - 1, CAP, CAP + 1 and 2 CAP + 1 (every row odd but at most one per window: R odd numbers sum to an even one);
    rows m / 2 .. m / 2 + 5 x 64 without any in-edge (whole wavefronts and whole workgroups of every geometry); the rest of the edges
    over the other rows in odd in-degrees (at most one even).  Returns (rows, windows = [(first row, R, total)])."""
    assert m % 2 == 0 and m >= 1024
    deg = np.zeros(m, dtype=np.int64)
    free = np.ones(m, dtype=bool)
    for h in (0, 5, m - 1):
        deg[h], free[h] = m - 1, False
    lo, hi = m // 2, m // 2 + 5 * 64
    free[lo:hi] = False
    windows = []
    at = 64
    for r in revs:
        R, CAP = r['R'], r['CAP']
        for tot in (CAP - 1, CAP, CAP + 1, 2 * CAP + 1):
            d = np.ones(R, dtype=np.int64)
            for _ in range((tot - R) // 2):
                d[rng.integers(0, R)] += 2
            d[rng.integers(0, R)] += (tot - R) % 2
            deg[at:at + R], free[at:at + R] = d, False
            windows.append((at, R, tot))
            at += R
        at = -(-at // 64) * 64
    assert at <= lo
    rest = np.nonzero(free)[0]
    left = m * K - int(deg.sum())
    d = np.ones(rest.size, dtype=np.int64)
    assert left >= rest.size
    extra = (left - rest.size) // 2
    d += 2 * (extra // rest.size)
    d[rng.choice(rest.size, extra % rest.size, replace=False)] += 2
    d[0] += (left - rest.size) % 2
    deg[rest] = d
    assert int(deg.sum()) == m * K
    src = np.repeat(np.arange(m), deg)
    return rng.permutation(src).reshape(1, m, K), windows


@pytest.mark.parametrize('H,K', [(4, 16), (8, 16), (16, 16), (32, 16), (64, 16), (8, 32), (32, 32)])
def test_reverse_walk_in_degrees(H, K):
    """The load-balanced reverse walks (bwd_rev_kernel, chain and final) over the in-degree plan of `indegree_rows`, m = 1024, k0 = 1,
    T = 3 (first walk, a chain walk reading the records, the final walk): hubs of in-degree >= m - 1 in the first and the last row,
    320 consecutive rows without an in-edge, odd in-degrees (pair sums straddle row boundaries), and R-aligned windows whose in-edges
    total CAP - 1, CAP, CAP + 1 and 2 CAP + 1 exactly -- all asserted on the table read back.  Column 0 is an arbitrary source here
    (k0 = 1 drops it by position; its edges are in the reverse list with weight 0).
    Bounds and CPU e32: BOUNDS['indeg'].
    Largest e measured on the MI355X: out 6.5e-07, dz 8.1e-07, dy 2.1e-06, dc 5.0e-07, dQ 1.3e-07, dP 1.6e-07."""
    m = 1024
    g = geometry(H)
    rng = np.random.default_rng(7 * H + K)
    plan, windows = indegree_rows(rng, m, K, g['REV'])
    tab = dense_table(plan, m)
    rows = device_rows(tab)
    indeg = torch.bincount(rows.reshape(-1), minlength=m)
    assert int(indeg[0]) == m - 1 and int(indeg[m - 1]) == m - 1 and int(indeg[5]) == m - 1
    assert int(indeg[m // 2:m // 2 + 320].sum()) == 0
    for at, R, tot in windows:
        assert at % R == 0 and int(indeg[at:at + R].sum()) == tot
    assert {tot for _, _, tot in windows} >= {r['CAP'] + d for r in g['REV'] for d in (-1, 0, 1)} | {2 * r['CAP'] + 1 for r in g['REV']}
    used = indeg[indeg > 0]
    assert int((used % 2 == 0).sum()) <= len(windows) + 1 and used.numel() > m // 2
    z, y, c, gout = mf_inputs(rng, m, H)
    mf_check('indeg', z, y, c, tab, 1, 3, gout)


# ------------------------------------------------------------------ 6: generic forms
DENSE_K = [(1, 0), (2, 1), (5, 0), (9, 1), (16, 0), (16, 2), (17, 1), (33, 1), (64, 0)]
KINDS = ['hub', 'dup', 'self', 'holes', 'empty', 'none', 'ragged']


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('H', NARROW)
def test_generic_forms(H, T):
    """The per-step kernels (sim / step kernels of crf.hip, bwd_edge + bwd_scatter and the similarity backward of crf_step_bwd.hip) at every
    width: dense NeighborTables with (K, k0) in DENSE_K (K = 1 and 64 the limits, 16 with k0 = 0 / 2 beside the fast shape, 17 and 33 one
    above the fast K), padded table_from_index tables in the kinds of shaped_rows (K = 9, k0 = 0: hub, duplicates, self-loops, interior
    holes, empty rows, no edge at all, ragged) and a table_from_edges table from a shuffled edge list (in-degrees 0 .. 12).  m = 151.
    None of them may take the restructured backward.  Bounds and CPU e32: BOUNDS['generic'].
    Largest e measured on the MI355X: out 9.9e-07, dz 5.6e-07, dy 1.3e-06, dc 9.5e-07, dQ 1.6e-07, dP 2.1e-07."""
    m = 151
    rng = np.random.default_rng(10 * H + T)
    z, y, c, gout = mf_inputs(rng, m, H)
    cases = [('dense', K, k0) for K, k0 in DENSE_K] + [(kind, 9, 0) for kind in KINDS] + [('edges', 12, 0)]
    for kind, K, k0 in cases:
        if kind == 'dense':
            tab = dense_table(knn_like(rng, 1, m, K), m)
        elif kind == 'edges':
            tab = edges_table(rng, m, tuple(range(13)))
        else:
            tab = index_table(shaped_rows(kind, rng, m, K))
        assert tab.K == K and tab.padded == (kind != 'dense') and supported(H, K, k0) == 0
        rows = device_rows(tab)
        if kind in ('empty', 'ragged', 'edges'):
            assert not (rows[m - 1] >= 0).any() and bool((rows >= 0).any())
        if kind == 'none':
            assert not (rows >= 0).any()
        mf_check('generic', z, y, c, tab, k0, T, gout)


# ------------------------------------------------------------------ 7: wide forms
@pytest.mark.parametrize('H', [65, 96, 128, 129, 200, 256])
def test_wide_forms(H):
    """The one-point-per-wavefront kernels of crf_wide.hip (4 rows per workgroup) at H = 128 / 256 and the padded widths 65, 96 (-> 128),
    129, 200 (-> 256); dc through _CrfMatricesWide (crf_matrices.hip: spd_inverse_wide_kernel), dQ / dP through _MeanFieldWide with leaf Q, P.
    m = 37 = 4 x 9 + 1, T = 3: dense K = 16 k0 = 1, dense K = 9 k0 = 0, padded K = 64 (`lane == k` at its limit) and the shaped_rows
    kinds at K = 9.  T = 0 and 1 on the dense K = 16 table; m = 1, 3, 4, 5 on the dense K = 9 table at T = 1.
    Bounds and CPU e32: BOUNDS['wide'].
    Largest e measured on the MI355X: out 1.2e-06, dz 1.2e-06, dy 1.7e-06, dc 1.5e-06, dQ 1.7e-07, dP 3.1e-07."""
    rng = np.random.default_rng(H)
    m = 37
    z, y, c, gout = mf_inputs(rng, m, H)
    d16 = dense_table(knn_like(rng, 1, m, 16), m)
    for T in (0, 1, 3):
        mf_check('wide', z, y, c, d16, 1, T, gout)
    mf_check('wide', z, y, c, dense_table(knn_like(rng, 1, m, 9), m), 0, 3, gout)
    r64 = rng.integers(0, m, (m, 64))
    r64[rng.random((m, 64)) < 0.1] = -1
    r64[:, 63] = (np.arange(m) + 1) % m
    mf_check('wide', z, y, c, index_table(r64), 0, 3, gout)
    for kind in KINDS:
        mf_check('wide', z, y, c, index_table(shaped_rows(kind, rng, m, 9)), 0, 3, gout)
    for m in (1, 3, 4, 5):
        z, y, c, gout = mf_inputs(rng, m, H)
        mf_check('wide', z, y, c, dense_table(knn_like(rng, 1, m, 9), m), 0, 1, gout)


# ------------------------------------------------------------------ 8: narrow padded widths
@pytest.mark.parametrize('H', [1, 3, 5, 12, 33, 63])
def test_narrow_padded_widths(H):
    """H below a kernel width: z, y, Q, P are zero-padded to 4 / 4 / 8 / 16 / 64 / 64 channels and the gradients come back in the
    unpadded shapes.  One fast table (K = 16, k0 = 1, B = 3 x 67 rows) and one padded ragged table (K = 9, k0 = 0), T = 3.
    Bounds and CPU e32: BOUNDS['padded'].
    Largest e measured on the MI355X: out 7.3e-07, dz 5.8e-07, dy 6.5e-07, dc 5.6e-07, dQ 1.2e-07, dP 2.0e-07."""
    B, n = 3, 67
    rng = np.random.default_rng(H)
    z, y, c, gout = mf_inputs(rng, B * n, H)
    mf_check('padded', z, y, c, dense_table(knn_like(rng, B, n, 16), n), 1, 3, gout)
    mf_check('padded', z, y, c, index_table(shaped_rows('ragged', rng, B * n, 9)), 0, 3, gout)


# ------------------------------------------------------------------ 9: input regimes
REGIMES = ['flat', 'underflow', 'identical', 'duplicate', 'tiny_gout', 'only_z', 'only_y', 'only_c', 'strided', 'expanded_gout', 'one_sided_gout']


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('H', [8, 32, 128])
def test_input_regimes(H, regime):
    """K = 16, k0 = 1, dense, B = 3 x 67 rows, T = 3, at one narrow in-launch-reduction width, one narrow stored-operand width and one
    wide width.  flat: y x 0.05 / 1.5 (all weights ~1 / 15).  underflow: two clusters of y rows whose squared distance exceeds 150, columns 1 .. 3 inside
    the cluster (weights >= 1e-3, asserted), columns 4 .. 15 across (float64 weight < 1e-60: exactly 0 in float32).  identical: every y
    row the same (uniform weights, exact ties; dy structurally zero).  duplicate: the same neighbour twice in every row.  tiny_gout:
    gout x 1e-6, every gradient still on its own scale.  only_z / only_y / only_c: one input requires grad, the others get None.
    strided: z, y and gout column slices of wider tensors.  expanded_gout: one row expanded with stride 0.  one_sided_gout: two
    channels of gout non-zero, rows scaled 0.5 .. 1.5.  Bounds and CPU e32: BOUNDS['regime'], BOUNDS['regime_g'].
    Largest e measured on the MI355X: regime: out 8.7e-07, dz 1.0e-06, dy 1.3e-06, dc 1.5e-06, dQ 1.6e-07, dP 2.3e-07;
    regime_g: out 8.8e-07, dz 6.2e-07, dy 7.5e-07, dc 4.6e-06, dQ 2.1e-07, dP 1.8e-07."""
    B, n, K = 3, 67, 16
    m = B * n
    rng = np.random.default_rng(sum(map(ord, regime)) + H)
    z, y, c, gout = mf_inputs(rng, m, H)
    plan = knn_like(rng, B, n, K)
    need = 'zym'
    if regime == 'flat':
        y = y * np.float32(0.05 / 1.5)
    elif regime == 'underflow':
        side = np.arange(n) % 2
        for b in range(B):
            for s in (0, 1):
                mine, other = np.nonzero(side == s)[0], np.nonzero(side != s)[0]
                plan[b, mine, 1:4] = rng.choice(mine, (mine.size, 3))
                plan[b, mine, 4:] = rng.choice(other, (mine.size, K - 4))
        y = y * np.float32(0.5)
        y[torch.from_numpy(np.tile(side, B) == 1)] += float(np.sqrt(200.0 / H))
    elif regime == 'identical':
        y = y[:1].expand(m, H).contiguous()
    elif regime == 'duplicate':
        plan[:, :, 5] = plan[:, :, 4]
    elif regime == 'tiny_gout':
        gout = gout * np.float32(1e-6)
    elif regime.startswith('only_'):
        need = {'z': 'z', 'y': 'y', 'c': 'm'}[regime[-1]]
    elif regime == 'strided':
        z, y, gout = (torch.cat([v, v], 1)[:, ::2] for v in (z, y, gout))          # the same values, row stride 2 H, column stride 2
        assert not z.is_contiguous()
    elif regime == 'expanded_gout':
        gout = gout[:1].expand(m, H)
    else:
        assert regime == 'one_sided_gout'
        e = torch.zeros(H)
        e[1], e[H - 1] = 1.0, 0.5
        gout = torch.linspace(0.5, 1.5, m)[:, None] * e[None]
    tab = dense_table(plan, n)
    rows = device_rows(tab)
    if regime == 'underflow':
        A, valid = ref_weights(y.double(), rows, 1)
        near = torch.tensor(np.tile(side, B))[rows] == torch.tensor(np.tile(side, B))[:, None]
        assert float(A[valid & near].min()) >= 1e-3 and float(A[valid & ~near].max()) < 1e-60 and int((valid & near).sum(1).min()) == 3
    if regime == 'duplicate':
        assert bool((rows[:, 1:-1] == rows[:, 2:]).any(1).all())
    if regime.startswith('only_'):
        r64 = mf_reference(z, y, c, rows, 1, 3, gout, torch.float64)
        r32 = mf_reference(z, y, c, rows, 1, 3, gout, torch.float32)
        got = mf_run(z, y, c, tab, 1, 3, gout, need=need)
        assert sorted(got) == sorted(['out', {'z': 'dz', 'y': 'dy', 'm': 'dc'}[need]])
        judge('regime', got, r32, r64)
        return
    # a gradient without a part along z: gQ - gP cancels to ~1 / sqrt(rows) of its terms and dc's float32 error grows with it (a site of its own)
    mf_check('regime_g' if regime in ('expanded_gout', 'one_sided_gout') else 'regime', z, y, c, tab, 1, 3, gout)


# ------------------------------------------------------------------ 10: the fast and the generic kernels on the same graph
@pytest.mark.parametrize('H', NARROW)
def test_fast_and_generic_forms_agree(H):
    """One fast-shape table (K = 16, k0 = 1, B = 3 x 67 rows) and its columns 1 .. 15 as a padded table at k0 = 0: the fast and the generic
    kernels on the same graph.  Each within its bound of float64, and within the SUM of the two bounds of each other (on the float64
    tensor's scale).  T = 3.  Bounds and CPU e32: BOUNDS['forms'].
    Largest e measured on the MI355X: out 6.0e-07, dz 4.9e-07, dy 6.1e-07, dc 6.2e-07, dQ 1.2e-07, dP 2.0e-07."""
    B, n, K = 3, 67, 16
    rng = np.random.default_rng(H)
    z, y, c, gout = mf_inputs(rng, B * n, H)
    fast = dense_table(knn_like(rng, B, n, K), n)
    slow = index_table(device_rows(fast)[:, 1:].numpy())
    assert supported(H, K, 1) == 1 and supported(H, K - 1, 0) == 0 and slow.padded
    a = mf_check('forms', z, y, c, fast, 1, 3, gout)
    b = mf_check('forms', z, y, c, slow, 0, 3, gout)
    for form in a:
        for k in a[form][0]:
            ref = a[form][2][k]
            e = float((a[form][0][k].double() - b[form][0][k].double()).abs().max() / ref.abs().max())
            print('[forms] %-4s fast vs generic %.3e' % (k, e), flush=True)
            assert e <= 2.0 * bound('forms', k), '%s: fast and generic forms differ by %.3e of the float64 scale' % (k, e)
