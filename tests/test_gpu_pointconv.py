"""-m gpu: ops.point_conv and ops.relpos_moments, form by form, against a float64 reference written here in plain torch with autograd on
the CPU -- the narrow statistics pass and its K tails (csrc/pointconv.hip: uvstats_body), the scalar wide loops in EB-edge batches split
over KS wavefronts (forward_kernel, uvstats_body, bwd_input_kernel; csrc/pointconv_bwd.hip: bwd_reduce_kernel, bwd_params_kernel,
bwd_dump_kernel, a1_reduce), the matrix-pipe kernels at K = 16 (csrc/pointconv_wide_stats.hip, csrc/pointconv_wide_params.hip), the
three ways the BatchNorm-2 statistics are finished (flat ticket, two-level ticket, no ticket + reduce_partials), BatchNorm-2's backward
reduction riding in the input-gradient launch (uv_bwd_reduce_body), the source-major walk of the reverse CSR, the folds and the moments
of csrc/pointconv_fold.hip, immediate and under ops.deferred_weight_grads (late slabs at d <= 16, _flush_pc_wide at d >= 32).

The reference (`pc_reference`) restates the layer on the edge list of the table AS THE DEVICE HOLDS IT (tab.idx32 read back, < 0 = no
neighbour):  rel = p_tgt[i] - p_src[j],  h = rel W1^T,  BatchNorm-1 (training: biased batch statistics over the valid edges; eval: the
running statistics),  LeakyReLU(slope),  W2^T,  BatchNorm-2 the same way,  out[i] = sum_k w_ik * x[j].  It returns out, dx and the six
parameter gradients, in training the four running tensors after the step (momentum 0.1, unbiased variance n / (n - 1), n = the valid
edges), and the rel-pos mean [3] and covariance [3, 3].  It runs once in float64 and once in float32; products whose inner dimension
is the edge count are formed in 64-row blocks (`rows_matmul`), so that the float32 run does not depend on a BLAS's summation order.

The LeakyReLU kink, by construction: no per-edge tensor is stored, so the kernel's own branch cannot be read back.  `nudge_beta1`
moves beta1 of every channel whose float64 layer-1 pre-activations come within TAU = 1e-4 of 0 by the nearest shift that leaves none
within TAU (gap midpoints and the points just outside the range), rounds to float32 and the test asserts min |pre| >= TAU over all valid
edges and channels (the float32 restatement's smallest |pre| is within 1e-6 of the float64 one in every case).  No channel is left out
of any comparison.

The comparison is test_gpu_discrete's `own_scale` on every tensor's OWN scale: e = max|got - ref64| / max|ref64| <= max(bound, 4 e32), and
e32 <= bound is asserted too.  A bound belongs to a SITE (test x tensor, BOUNDS below) and is ~10 x the largest e32 the float32
restatement showed on the CPU over that site's cases (the factor: another summation order).  Inputs are scaled for it: positions in a
unit box, W2 / sqrt(d), gamma in 0.5 .. 1.5, x and gout with means away from 0.  Structural zeros are exact zeros: the out rows of targets
without a valid entry, the dx rows of sources without an in-edge.  No tensor of these cases is zero by cancellation alone: the one-row
cases are bipartite (one target over K + 1 sources, seven targets over one source), so that rel differs between the edges and neither
BatchNorm sees a constant; a channel of dbeta1 whose pre-activations all have one sign does cancel (BatchNorm-2 removes a constant shift
of h2), but the tensor is judged by its largest channel.  In eval mode the running statistics and num_batches_tracked must be
bit-identical before and after.  Before every forward and backward the allocator is poisoned with NaN blocks of the outputs' shapes, every
output is asserted finite, and for every case the rule must refuse each tensor zeroed and mis-scaled by 10 x its bound (arithmetic on
results already computed, no launch).  Which entries of the library ran is RECORDED (`recorded`) and asserted per case.

The kernels' geometry is READ from the sources (`geometry`): macro defaults and constants by name, the formulas restated beside them; each
case asserts the property it is named for, so a change of a tunable moves the cases with it.

Beyond the table forms of the dense, ragged (table_from_edges) and bipartite cases, test_holes_anywhere puts -1 entries in FRONT of valid
ones (table_from_index), which no left-packed table does.

Left out on purpose: the rider launch forward_uv_hosting and point_conv_prefold (test_gpu_model.py), the operand-load combine
(test_gpu_operand_fold.py), state.no_wide128 (test_gpu_backward_tail.py).  Measured figures per site: BOUNDS and
profiles/r27_pointconv_float64.md."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import DEV, t
from test_gpu_discrete import dev, device_rows, edges_table, f32, index_table, leaf, own_scale, poison, rejected, shaped_rows

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crfconv_amd', 'csrc')
WIDTHS = (4, 8, 16, 32, 64, 128)
TAU, EPS, MOM = 1e-4, 1e-5, 0.1
GRADS = ('dx', 'dW1', 'dgamma1', 'dbeta1', 'dW2', 'dgamma2', 'dbeta2')
RUNNING = ('rm1', 'rv1', 'rm2', 'rv2')

# site -> tensor -> (bound, largest e32 of the float32 restatement on the CPU, largest e measured on the MI355X); bound ~ 10 x e32.
# A site is the group of cases of the test named beside it, all widths.  No bound is below 1e-6 = 16 float32 roundings: where the
# float32 restatement came within one or two roundings of float64 (a [3] mean, a running tensor whose every entry is one rounded
# number), ten times that figure would measure the luck of one summation order, not the kernel.
BOUNDS = {
    'widths': dict(out=(5e-06, 6.0e-07, 4.7e-07), dx=(7e-06, 8.0e-07, 6.0e-07), dW1=(2e-05, 1.6e-06, 1.3e-06), dgamma1=(3e-05, 2.2e-06, 9.4e-06),
                   dbeta1=(7e-05, 6.2e-06, 2.6e-05), dW2=(2e-05, 2.1e-06, 5.5e-06), dgamma2=(2e-05, 1.5e-06, 4.1e-06), dbeta2=(2e-06, 1.6e-07, 6.4e-07),
                   rm1=(2e-06, 1.0e-07, 7.9e-08), rv1=(1e-06, 9.4e-08, 5.5e-08), rm2=(2e-06, 1.2e-07, 9.1e-08), rv2=(2e-06, 1.0e-07, 6.1e-08),
                   mean=(6e-06, 1.1e-06, 2.8e-06), cov=(2e-06, 1.6e-07, 1.3e-07)),
    'eval': dict(out=(4e-06, 3.3e-07, 2.9e-07), dx=(3e-06, 2.2e-07, 2.7e-07), dW1=(4e-06, 3.5e-07, 2.3e-07), dgamma1=(3e-06, 2.7e-07, 1.6e-07),
                 dbeta1=(2e-06, 1.5e-07, 9.0e-08), dW2=(3e-06, 3.6e-07, 2.4e-07), dgamma2=(3e-06, 2.5e-07, 2.4e-07), dbeta2=(2e-06, 1.4e-07, 1.0e-07),
                 mean=(2e-05, 1.2e-06, 9.8e-07), cov=(2e-06, 1.1e-07, 8.8e-08)),
    'rows': dict(out=(2e-05, 1.8e-06, 1.9e-06), dx=(2e-05, 1.4e-06, 1.4e-06), dW1=(3e-05, 2.6e-06, 3.1e-06), dgamma1=(9e-05, 8.6e-06, 1.1e-05),
                 dbeta1=(5e-05, 4.2e-06, 1.2e-05), dW2=(4e-05, 3.5e-06, 8.7e-06), dgamma2=(3e-05, 2.7e-06, 2.4e-06), dbeta2=(3e-06, 2.3e-07, 4.9e-07),
                 rm1=(2e-06, 1.6e-07, 7.6e-08), rv1=(1e-06, 1.0e-07, 8.5e-08), rm2=(2e-06, 1.9e-07, 2.4e-07), rv2=(2e-06, 1.2e-07, 1.9e-07),
                 mean=(6e-06, 5.2e-07, 1.1e-06), cov=(2e-06, 1.4e-07, 1.3e-06)),
    'finish': dict(out=(2e-05, 1.4e-06, 1.3e-06), dx=(2e-05, 1.0e-06, 9.7e-07), dW1=(2e-05, 2.2e-06, 3.0e-06), dgamma1=(6e-05, 5.7e-06, 3.4e-06),
                   dbeta1=(2e-04, 1.9e-05, 2.1e-05), dW2=(5e-05, 4.9e-06, 1.2e-05), dgamma2=(5e-05, 6.2e-06, 8.3e-06), dbeta2=(2e-06, 1.7e-07, 4.2e-07),
                   rm1=(2e-06, 1.1e-07, 5.3e-08), rv1=(2e-06, 1.0e-07, 4.7e-08), rm2=(2e-06, 1.2e-07, 5.1e-08), rv2=(2e-06, 1.1e-07, 5.5e-08),
                   mean=(2e-05, 1.3e-06, 4.4e-07), cov=(2e-06, 2.0e-07, 9.1e-08)),
    'padded': dict(out=(4e-06, 4.2e-07, 3.6e-07), dx=(8e-06, 7.4e-07, 7.4e-07), dW1=(2e-05, 1.2e-06, 6.0e-07), dgamma1=(1e-05, 1.2e-06, 1.6e-06),
                   dbeta1=(3e-05, 2.2e-06, 3.4e-06), dW2=(2e-05, 1.5e-06, 2.8e-06), dgamma2=(2e-05, 1.4e-06, 1.1e-06), dbeta2=(2e-06, 1.2e-07, 2.7e-07),
                   rm1=(2e-06, 1.2e-07, 4.4e-08), rv1=(1e-06, 8.7e-08, 4.2e-08), rm2=(2e-06, 1.3e-07, 4.5e-08), rv2=(2e-06, 1.0e-07, 4.8e-08),
                   mean=(2e-06, 1.4e-07, 7.1e-08), cov=(2e-06, 1.1e-07, 4.4e-08)),
    'regime': dict(out=(4e-06, 4.6e-07, 3.3e-07), dx=(5e-06, 5.7e-07, 4.5e-07), dW1=(3e-06, 3.2e-07, 2.6e-07), dgamma1=(4e-06, 8.7e-07, 9.6e-07),
                   dbeta1=(1e-05, 9.8e-07, 1.1e-06), dW2=(6e-06, 8.5e-07, 9.0e-07), dgamma2=(3e-06, 3.4e-07, 4.0e-07), dbeta2=(4e-05, 4.0e-06, 6.2e-06),
                   rm1=(1e-06, 9.2e-08, 4.4e-08), rv1=(1e-06, 9.9e-08, 4.4e-08), rm2=(1e-06, 9.1e-08, 4.5e-08), rv2=(1e-06, 9.6e-08, 4.1e-08),
                   mean=(1e-06, 2.2e-08, 3.6e-07), cov=(1e-06, 8.6e-08, 6.3e-08)),
    'moments': dict(rm1=(5e-06, 4.3e-07, 2.1e-07), rv1=(2e-06, 1.5e-07, 9.2e-08), rm2=(2e-06, 1.9e-07, 8.7e-08), rv2=(2e-06, 1.2e-07, 1.5e-07),
                    mean=(3e-06, 2.6e-07, 1.8e-07), cov=(1e-06, 9.4e-08, 5.0e-08)),
    'holes': dict(out=(4e-06, 3.8e-07, 3.6e-07), dx=(4e-06, 4.1e-07, 3.0e-07), dW1=(4e-06, 4.6e-07, 7.3e-07), dgamma1=(4e-06, 7.4e-07, 1.8e-06),
                  dbeta1=(8e-06, 1.0e-06, 2.0e-06), dW2=(5e-06, 8.3e-07, 2.0e-06), dgamma2=(6e-06, 7.1e-07, 2.6e-06), dbeta2=(2e-06, 1.2e-07, 4.1e-07),
                  rm1=(1e-06, 8.8e-08, 4.7e-08), rv1=(2e-06, 1.1e-07, 4.2e-08), rm2=(1e-06, 7.4e-08, 4.3e-08), rv2=(2e-06, 1.2e-07, 4.5e-08),
                  mean=(2e-06, 1.9e-07, 1.8e-07), cov=(2e-06, 1.1e-07, 9.9e-08)),
}


def bound(site, name):
    return BOUNDS[site][name][0]


# ------------------------------------------------------------------ the kernels' geometry, read from the sources
def _src(fname):
    return open(os.path.join(CSRC, fname)).read()


def _csrc_int(fname, name):
    """The integer a source file gives `name`: `#define name N` (the default under #ifndef) or `constexpr int name = N;`."""
    text = _src(fname)
    hit = re.search(r'#define\s+%s\s+(\d+)' % name, text) or re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert hit, '%s: no %s' % (fname, name)
    return int(hit.group(1))


def geometry(d):
    """Rows per workgroup and the forks of the PointConv kernels at width d, the formulas of the sources restated:
    PC<D>: L = D / 4, PPW = WAVE / L, KS = PC_KS_<D> (1 below 32), PPB = PPW (PBLOCK / WAVE) / KS, EB = D >= 32 ? 4 : 1   (pointconv_common.hpp)
    UG = UV_GROUP edges per trip of the narrow statistics pass                                                        (pointconv_common.hpp)
    last_workgroup_of: flat ticket up to LW_FLAT workgroups, above it LW_GROUPS groups                                       (gridsync.hpp)
    crfconv_pointconv_forward_uv: no ticket when nblk (d / 2) > NT                                                          (pointconv.hip)
    uv_reduce_blocks: rpi = 256 / (d / 4) rows per trip, RED_TRIPS rows per thread, at most RED_MAX workgroups              (pointconv.hip)
    matrix-pipe kernels, K = 16: WP_WAVES = WP_BLOCK / WAVE wavefronts of wide_points_per_wave(m) points each   (pointconv_wide.hpp,
    pointconv_wide_stats.hip: uvstats_mfma_launch); the d = 128 parameter pass: 256 dumped edge rows = 16 points (pointconv_wide_params.hip)."""
    wave = 64
    common, conv, wide = _src('pointconv_common.hpp'), _src('pointconv.hip'), _src('pointconv_wide.hpp')
    pblock = _csrc_int('pointconv_common.hpp', 'PBLOCK')
    L = d // 4
    assert re.search(r'KS = D >= 128 \? PC_KS_128 : \(D >= 64 \? PC_KS_64 : \(D >= 32 \? PC_KS_32 : 1\)\)', common)
    assert re.search(r'PPB = PPW \* PWAVES / KS;', common) and re.search(r'EB = \(D >= 32\) \? 4 : 1;', common)
    KS = 1 if d < 32 else _csrc_int('pointconv_common.hpp', 'PC_KS_%d' % d)
    g = dict(L=L, PPW=wave // L, KS=KS, PPB=wave // L * (pblock // wave) // KS, EB=4 if d >= 32 else 1,
             UG=_csrc_int('pointconv_common.hpp', 'UV_GROUP'), LW_FLAT=_csrc_int('gridsync.hpp', 'LASTWG_FLAT_'),
             LW_GROUPS=_csrc_int('gridsync.hpp', 'LASTWG_GROUPS_'))
    hit = re.search(r'if \(nblk \* \(d / 2\) > (\d+) \* (\d+)\) ticket = nullptr;', conv)
    assert hit, 'pointconv.hip: no no-ticket rule'
    g['NT'] = int(hit.group(1)) * int(hit.group(2))
    hit = re.search(r'const int rpi = 256 / \(d / 4\);\s*const int64_t nb = cdiv\(m, \(int64_t\)rpi \* (\d+)\);[^\n]*\n\s*'
                    r'return nb < 1 \? 1 : \(nb > (\d+) \? \2 : nb\);', conv)
    assert hit, 'pointconv.hip: no uv_reduce_blocks'
    g['RPI'], g['RED_TRIPS'], g['RED_MAX'] = 256 // L, int(hit.group(1)), int(hit.group(2))
    hit = re.search(r'return m_tgt >= (\d+) \? WP_PPW_BIG_ : \(m_tgt >= (\d+) \? WP_PPW_MID_ : WP_PPW_SMALL_\);', wide)
    assert hit, 'pointconv_wide.hpp: no wide_points_per_wave'
    g['WP_WAVES'] = _csrc_int('pointconv_wide.hpp', 'WP_BLOCK_') // wave
    g['WP_PPW'] = ((int(hit.group(1)), _csrc_int('pointconv_wide.hpp', 'WP_PPW_BIG_')), (int(hit.group(2)), _csrc_int('pointconv_wide.hpp', 'WP_PPW_MID_')),
                   (0, _csrc_int('pointconv_wide.hpp', 'WP_PPW_SMALL_')))
    assert re.search(r'cdiv\(m_tgt, wide_points_per_wave\(m_tgt\) \* WP_WAVES\)', _src('pointconv_wide_stats.hip'))
    assert re.search(r'd == 128 \? wg_plan\(m_tgt \* 16, 128, 128\)\.nblk', _src('pointconv_wide_params.hip'))
    return g


def nblocks(g, m):
    return -(-m // g['PPB'])


def wide_points(g, m):
    """Points per workgroup of the matrix-pipe statistics kernel over m targets."""
    return [p for lo, p in g['WP_PPW'] if m >= lo][0] * g['WP_WAVES']


def stats_finish(g, d, K, m):
    """(kernel, workgroups, how the BatchNorm-2 statistics are finished) of crfconv_pointconv_forward_uv over m targets."""
    if K == 16 and d >= 32:
        n = max(1, -(-m // wide_points(g, m)))
        return 'mfma', n, 'flat' if n <= g['LW_FLAT'] else 'two-level'
    n = nblocks(g, m)
    return 'scalar', n, 'none' if n * (d // 2) > g['NT'] else ('flat' if n <= g['LW_FLAT'] else 'two-level')


def reduce_blocks(g, m):
    return min(max(-(-m // (g['RPI'] * g['RED_TRIPS'])), 1), g['RED_MAX'])


def reduce_trips(g, m):
    """Row trips per thread of uv_bwd_reduce_body over m rows: the set over all threads of all its workgroups."""
    stride = reduce_blocks(g, m) * g['RPI']
    return {-(-(m - r0) // stride) for r0 in range(min(stride, m))} | ({0} if m < stride else set())


# ------------------------------------------------------------------ float64 / float32 reference (plain torch, autograd)
def rows_matmul(x, M, blk=64):
    """x M for x [E, a], M [a, b], as a batch of 64-row blocks against the expanded M: the gradient of M is then a sum of per-block
    products over the block axis (torch.sum: a cascade), not one product with inner dimension E whose float32 summation order is the
    BLAS's own (test_gpu_meanfield.rows_matmul, for any a, b)."""
    E, a = x.shape
    n = -(-E // blk)
    xp = torch.nn.functional.pad(x, (0, 0, 0, n * blk - E)) if n * blk != E else x
    return torch.bmm(xp.view(n, blk, a), M.expand(n, a, M.shape[1])).reshape(n * blk, M.shape[1])[:E]


def edge_list(rows):
    ti, tk = (rows >= 0).nonzero(as_tuple=True)
    return ti, rows[ti, tk]


def pre_activations(inp, rows, train, dtype):
    """Layer-1 pre-activations [edges, d] of the valid edges (no autograd)."""
    with torch.no_grad():
        c = lambda k: inp[k].to(dtype)
        ti, sj = edge_list(rows)
        h = rows_matmul(c('pt')[ti] - c('ps')[sj], c('W1').t())
        mu, var = (h.mean(0), h.var(0, unbiased=False)) if train else (c('rm1'), c('rv1'))
        return (h - mu) / torch.sqrt(var + EPS) * c('g1') + c('b1')


def pc_reference(inp, rows, train, dtype):
    """{out, dx, dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2, mean, cov} and, in training, {rm1, rv1, rm2, rv2} after the step."""
    c = lambda k: inp[k].to(dtype)
    x, W1, g1, b1, W2, g2, b2 = (leaf(inp[k], dtype) for k in ('x', 'W1', 'g1', 'b1', 'W2', 'g2', 'b2'))
    ti, sj = edge_list(rows)
    n = ti.numel()
    rel = c('pt')[ti] - c('ps')[sj]
    slope = inp['slope']

    def bn(h, gamma, beta, rm, rv):
        mu, var = (h.mean(0), h.var(0, unbiased=False)) if train else (rm, rv)
        return (h - mu) / torch.sqrt(var + EPS) * gamma + beta, mu.detach(), var.detach()
    pre, mu1, var1 = bn(rows_matmul(rel, W1.t()), g1, b1, c('rm1'), c('rv1'))
    w, mu2, var2 = bn(rows_matmul(torch.nn.functional.leaky_relu(pre, slope), W2.t()), g2, b2, c('rm2'), c('rv2'))
    out = torch.zeros(rows.shape[0], x.shape[1], dtype=dtype).index_add(0, ti, w * x[sj])
    (out * c('gout')).sum().backward()
    res = dict(out=out.detach())
    for k, v in zip(GRADS, (x, W1, g1, b1, W2, g2, b2)):
        res[k] = torch.zeros_like(v) if v.grad is None else v.grad
    mean = rel.mean(0)
    rc = rel - mean
    res['mean'], res['cov'] = mean, (rc[:, :, None] * rc[:, None, :]).mean(0)
    if train:
        unb = n / (n - 1.0)
        for k, old, new in (('rm1', c('rm1'), mu1), ('rv1', c('rv1'), var1 * unb), ('rm2', c('rm2'), mu2), ('rv2', c('rv2'), var2 * unb)):
            res[k] = (1.0 - MOM) * old + MOM * new
    res['_pre_min'] = float(pre.detach().abs().min())
    return res


def nudge_beta1(inp, rows, train):
    """beta1 (BatchNorm-1's bias, in both modes) moved so that no float64 layer-1 pre-activation of a valid edge is within TAU of 0: per
    channel that comes within TAU, subtract the z nearest 0 among the midpoints of the gaps of at least 2.2 TAU between neighbouring
    pre-activations and the points 1.1 TAU outside their range.  Returns (channels moved, largest |z|, min |pre| after)."""
    pre = pre_activations(inp, rows, train, torch.float64)
    b = inp['b1'].double().clone()
    moved, zmax = 0, 0.0
    for ch in (pre.abs().min(0).values < 1.05 * TAU).nonzero().reshape(-1).tolist():
        p = pre[:, ch].sort().values
        gaps = p[1:] - p[:-1]
        ok = gaps >= 2.2 * TAU
        cand = torch.cat([((p[1:] + p[:-1]) / 2)[ok], p[:1] - 1.1 * TAU, p[-1:] + 1.1 * TAU])
        z = float(cand[cand.abs().argmin()])
        b[ch] -= z
        moved, zmax = moved + 1, max(zmax, abs(z))
    inp['b1'] = b.float()
    return moved, zmax, float(pre_activations(inp, rows, train, torch.float64).abs().min())


# ------------------------------------------------------------------ inputs and tables
def pc_inputs(rng, m_src, m_tgt, d, bipartite, slope=0.1):
    """Positions in a unit box; W1 ~ N(0, 1), W2 ~ N(0, 1) / sqrt(d); gamma in 0.5 .. 1.5, beta in -0.5 .. 0.5; running means in -0.2 .. 0.2,
    running variances in 0.3 .. 0.8 (h = rel W1^T) and 0.5 .. 1.5; x in -0.5 .. 1 and gout = 0.3 + 0.5 N(0, 1): means away from 0, so that
    dbeta2 = sum g x and the d x d sums do not cancel."""
    ps = f32(rng, (m_src, 3), 0.0, 1.0)
    nrm = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return dict(ps=ps, pt=f32(rng, (m_tgt, 3), 0.0, 1.0) if bipartite else ps, x=f32(rng, (m_src, d), -0.5, 1.0),
                gout=0.3 + 0.5 * nrm(m_tgt, d), W1=nrm(d, 3), W2=nrm(d, d) / np.float32(np.sqrt(d)),
                g1=f32(rng, (d,), 0.5, 1.5), b1=f32(rng, (d,), -0.5, 0.5), g2=f32(rng, (d,), 0.5, 1.5), b2=f32(rng, (d,), -0.5, 0.5),
                rm1=f32(rng, (d,), -0.2, 0.2), rv1=f32(rng, (d,), 0.3, 0.8), rm2=f32(rng, (d,), -0.2, 0.2), rv2=f32(rng, (d,), 0.5, 1.5),
                slope=slope)


def self_rows(rng, m, K):
    """[m, K] over the same m points: column 0 the row itself (self edges: rel = 0), the last column of every third row a repeat of
    another column's source, the rest anywhere."""
    rows = rng.integers(0, m, (m, K))
    rows[:, 0] = np.arange(m)
    if K > 2:
        rows[::3, K - 1] = rows[::3, 1]
    return rows


def self_table(rows):
    """Dense NeighborTable of one cloud (the device re-sorts columns 1..; uint16 ids beside int32 when K % 8 == 0)."""
    from crfconv_amd.graph import NeighborTable
    return NeighborTable(t(np.asarray(rows)[None].astype(np.int64)), rows.shape[0])


def bipartite_rows(rows, m_src):
    """int [m_tgt, K] rows over m_src sources without holes -> padded = True table (graph.table_from_index; every entry an edge)."""
    from crfconv_amd.graph import table_from_index
    rows = np.asarray(rows)
    assert rows.min() >= 0 and rows.max() < m_src
    return table_from_index(t(np.ascontiguousarray(rows.astype(np.int32))), m_src)


def ragged_plan(rng, m_tgt, m_src, K, hub=220, dead=8):
    """Edge list (tgt, src) for table_from_edges: entries per target drawn from {0, 1, 3, K} (each occurs, the last target has none); source 0
    a hub of `hub` edges; the last `dead` sources without an in-edge; shuffled."""
    deg = rng.choice(np.array([0, 1, 3, K]), m_tgt)
    deg[:4], deg[-1] = (0, 1, 3, K), 0
    tgt = np.repeat(np.arange(m_tgt), deg)
    src = rng.integers(1, m_src - dead, tgt.size)
    src[rng.choice(tgt.size, hub, replace=False)] = 0
    perm = rng.permutation(tgt.size)
    return tgt[perm], src[perm]


def ragged_table(rng, m_tgt, m_src, K):
    from crfconv_amd.graph import table_from_edges
    tgt, src = ragged_plan(rng, m_tgt, m_src, K)
    tab = table_from_edges(t(tgt), t(src), m_tgt, m_src)
    rows = device_rows(tab)
    indeg = torch.bincount(rows[rows >= 0], minlength=m_src)
    assert tab.padded and tab.K == K and tab.n_edges == tgt.size == int((rows >= 0).sum())
    assert int(indeg[0]) >= 200 and int(indeg[-8:].sum()) == 0 and not (rows[-1] >= 0).any()
    assert set((rows >= 0).sum(1).tolist()) == {0, 1, 3, K}
    return tab


# ------------------------------------------------------------------ the layer on the device
@contextlib.contextmanager
def recorded(names):
    """The names of the library entries called through crfconv_amd._lib.call inside the block, appended to `names`."""
    from crfconv_amd import _lib
    inner = _lib.call

    def call(name, *args):
        names.append(name)
        return inner(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = inner


def pc_run(inp, tab, train, deferred=False):
    """ops.relpos_moments + ops.point_conv forward + backward on the host tensors of `inp`.  Returns (results, entries called)."""
    from crfconv_amd import ops
    d = inp['x'].shape[1]
    m_tgt, m_src = inp['pt'].shape[0], inp['ps'].shape[0]
    W1, W2 = torch.nn.Parameter(dev(inp['W1'])), torch.nn.Parameter(dev(inp['W2']))
    bns = []
    for g, b, rm, rv in (('g1', 'b1', 'rm1', 'rv1'), ('g2', 'b2', 'rm2', 'rv2')):
        bn = torch.nn.BatchNorm1d(d, eps=EPS, momentum=MOM).to(DEV).train(train)
        with torch.no_grad():
            bn.weight.copy_(inp[g]); bn.bias.copy_(inp[b]); bn.running_mean.copy_(inp[rm]); bn.running_var.copy_(inp[rv])
        bns.append(bn)
    before = [(bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in bns]
    x = dev(inp['x']).requires_grad_(True)
    ps = dev(inp['ps'])
    pt = ps if inp['pt'] is inp['ps'] else dev(inp['pt'])
    names = []
    with recorded(names):
        poison((m_tgt, d), (m_tgt, d), (m_tgt, d), (d, 3), (d,), (2 * d,))
        mom = ops.relpos_moments(ps, pt, tab)
        out = ops.point_conv(x, ps, pt, tab, W1, bns[0], W2, bns[1], train, moments=mom, slope=inp['slope'])
        assert out.shape == (m_tgt, d)
        poison((m_src, d), (5, d), (d, d), (d, 4), (d, 3), (d,), (d,), (m_tgt, d), (m_tgt, d))
        with ops.deferred_weight_grads(enabled=deferred):
            out.backward(dev(inp['gout']))
        torch.cuda.synchronize()
    res = dict(out=out.detach().cpu(), mean=mom[0].cpu(), cov=mom[1].cpu())
    for k, v in zip(GRADS, (x, W1, bns[0].weight, bns[0].bias, W2, bns[1].weight, bns[1].bias)):
        assert v.grad is not None and tuple(v.grad.shape) == tuple(v.shape), k
        res[k] = v.grad.cpu()
    for bn, (rm, rv, nbt), keys in zip(bns, before, (RUNNING[:2], RUNNING[2:])):
        if train:
            res[keys[0]], res[keys[1]] = bn.running_mean.cpu(), bn.running_var.cpu()
            assert int(bn.num_batches_tracked) == int(nbt) + 1
        else:
            assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and torch.equal(bn.num_batches_tracked, nbt), \
                'eval mode moved the running statistics'
    return res, names


def entries_expected(lib, d, K, m_tgt, train, deferred):
    """The PointConv entries a case must and must not reach (ops/pointconv.py, ops/defer.py)."""
    from crfconv_amd import ops
    P = 'crfconv_pointconv_'
    if train:
        yes, no = [P + 'forward_uv', P + 'combine', P + 'bwd_input_reduce'], [P + 'forward', P + 'bwd_input', P + 'bwd_reduce', P + 'fold2_bwd']
    else:
        yes, no = [P + 'fold2', P + 'forward', P + 'bwd_input', P + 'bwd_reduce', P + 'fold2_bwd'], [P + 'forward_uv', P + 'combine', P + 'bwd_input_reduce']
    if d <= 16:                                                        # in-kernel sums, or the late slabs
        yes += [P + 'bwd_params'] + ([P + 'bwd_params_slabs'] if deferred else [])
        no += [P + 'bwd_dump', P + 'bwd_dump_jobs', P + 'wide_params_jobs'] + ([] if deferred else [P + 'bwd_params_slabs'])
    elif not deferred:                                                 # the dump path, immediate
        yes += [P + 'bwd_dump', P + 'bwd_a1']
        no += [P + 'bwd_params', P + 'bwd_dump_jobs', P + 'wide_params_jobs']
    elif lib.crfconv_pointconv_wide_params_supported(m_tgt, K, d) == 1 and not ops.state.no_wide128:        # the matrix pipe
        yes += [P + 'wide_params_jobs']
        no += [P + 'bwd_params', P + 'bwd_dump', P + 'bwd_dump_jobs', P + 'bwd_a1_jobs']
    else:                                                              # the dump path, batched at the end of the pass
        yes += [P + 'bwd_dump_jobs', P + 'bwd_a1_jobs']
        no += [P + 'bwd_params', P + 'bwd_dump', P + 'wide_params_jobs']
    yes.append(P + ('fold1_bwd_batched' if deferred else 'fold1_bwd'))
    return yes, no


def judge(site, got, r32, r64, rows, m_src):
    """Every tensor of `got` against float64 on its own scale within the site's bound; exact zeros in the out rows of targets without a
    valid entry and the dx rows of sources without an in-edge; the rule refuses each tensor zeroed and mis-scaled by 10 x its bound."""
    assert set(got) == set(k for k in r64 if not k.startswith('_')), sorted(set(got) ^ set(r64))
    for k in sorted(got):
        g = got[k].detach().cpu()
        b = bound(site, k)
        own_scale(g, r32[k], r64[k], b, site + '.' + k)
        assert rejected(torch.zeros_like(g), r32[k], r64[k], b), '%s.%s zeroed passes' % (site, k)
        assert rejected(g.double() * (1.0 + 10.0 * b), r32[k], r64[k], b), '%s.%s mis-scaled by 10 x the bound passes' % (site, k)
    empty = ~(rows >= 0).any(1)
    unused = torch.bincount(rows[rows >= 0], minlength=m_src) == 0
    if 'out' in got:
        assert bool((got['out'][empty] == 0).all()), '%s: out of a target without a valid entry is not zero' % site
        assert bool((got['dx'][unused] == 0).all()), '%s: dx of a source without an in-edge is not zero' % site


def pc_check(site, inp, tab, train, deferred=(False,), only=None):
    """One case: nudge, both references, the device run(s), the comparison.  only: the tensors compared (all by default).
    Returns (rows, {deferred: entries called})."""
    from crfconv_amd import _lib
    rows = device_rows(tab)
    m_tgt, m_src, d = inp['pt'].shape[0], inp['ps'].shape[0], inp['x'].shape[1]
    assert tuple(rows.shape) == (m_tgt, tab.K) and int(rows.max()) < m_src and tab.m_src == m_src and tab.m_tgt == m_tgt
    assert tab.n_edges == int((rows >= 0).sum()) >= 2
    moved, zmax, pre_min = nudge_beta1(inp, rows, train)
    r64 = pc_reference(inp, rows, train, torch.float64)
    r32 = pc_reference(inp, rows, train, torch.float32)
    print('[kink] %s d %d: %d channels moved (largest %.1e), min |pre| %.3e (float32 %.3e)' % (site, d, moved, zmax, pre_min, r32['_pre_min']), flush=True)
    assert pre_min >= TAU and r64['_pre_min'] >= TAU and r32['_pre_min'] >= 0.9 * TAU
    called = {}
    for df in deferred:
        got, names = pc_run(inp, tab, train, df)
        yes, no = entries_expected(_lib.load(), d, tab.K, m_tgt, train, df)
        assert all(n in names for n in yes) and not any(n in names for n in no), (df, [n for n in yes if n not in names], [n for n in no if n in names])
        if only is not None:
            got = {k: got[k] for k in only}
            judge(site, got, r32, {k: r64[k] for k in only}, rows, m_src)
        else:
            judge(site, got, r32, r64, rows, m_src)
        called[df] = names
    return rows, called


def seed(*parts):
    return np.random.default_rng([int(p) for p in parts])


# ------------------------------------------------------------------ 1: every width at every K fork
KS_OF_TEST_1 = (2, 3, 4, 6, 16, 17, 64)


@pytest.mark.parametrize('K', KS_OF_TEST_1)
@pytest.mark.parametrize('d', WIDTHS)
def test_widths_and_k(d, K):
    """Dense self table (column 0 the row itself, repeated sources in every third row), m = 2 PPB + 3 (three workgroups, the last of three
    rows), training.  K = 2, 3, 6, 17: tails of the UV_GROUP = 4 trips (d <= 16) and of the EB = 4 batches (d >= 32); K = 2, 3, 4, 6 < KS EB
    at d = 64: wavefronts of a group without an edge or with a tail only; 16: the matrix-pipe statistics pass at d >= 32; 64: the limit.
    Immediate, and under deferred weight gradients at K = 3, 16, 17: late slabs (d <= 16), the batched dump path (d >= 32, K = 3, 17), the
    matrix-pipe parameter pass (d >= 32, K = 16) -- which entries ran is asserted (`entries_expected`).  Bounds and CPU e32: BOUNDS['widths']."""
    g = geometry(d)
    m = 2 * g['PPB'] + 3
    assert nblocks(g, m) == 3 and (K % g['UG'] != 0 or K % g['EB'] != 0) == (K in (2, 3, 6, 17))
    if d == 64:
        assert (K < g['KS'] * g['EB']) == (K <= 6) and g['KS'] == 4
    rng = seed(1, d, K)
    tab = self_table(self_rows(rng, m, K))
    assert not tab.padded and (tab.idx16 is not None) == (K % 8 == 0)
    assert stats_finish(g, d, K, m)[0] == ('mfma' if K == 16 and d >= 32 else 'scalar')
    inp = pc_inputs(rng, m, m, d, False)
    rows, _ = pc_check('widths', inp, tab, True, (False, True) if K in (3, 16, 17) else (False,))
    assert bool((rows[:, 0] == torch.arange(m)).all())
    if K > 2:
        by_source = rows.sort(1).values
        assert bool((by_source[:, 1:] == by_source[:, :-1]).any(1)[::3].all())


# ------------------------------------------------------------------ 2: eval mode
@pytest.mark.parametrize('K', [5, 16])
@pytest.mark.parametrize('d', WIDTHS)
def test_eval_mode(d, K):
    """Both BatchNorms on running statistics drawn away from (0, 1): fold1 / fold2 with use_batch = 0, forward_kernel, bwd_input without
    the riding reduction, bwd_reduce_kernel, fold2_bwd -- at K = 5 (tails everywhere; also under deferred weight gradients) and K = 16
    (the matrix-pipe parameter pass reads eval-mode coefficients under deferral at d >= 32).  Dense self table, m = 2 PPB + 3.  The
    running statistics and num_batches_tracked are bit-identical afterwards (pc_run).  Bounds and CPU e32: BOUNDS['eval']."""
    g = geometry(d)
    m = 2 * g['PPB'] + 3
    rng = seed(2, d, K)
    tab = self_table(self_rows(rng, m, K))
    inp = pc_inputs(rng, m, m, d, False)
    pc_check('eval', inp, tab, False, (False, True))


# ------------------------------------------------------------------ 3: row counts
def row_count_cases(d):
    """(K, m_tgt, m_src, deferred) of test_row_counts at width d."""
    g = geometry(d)
    P = g['PPB']
    cases = [(4, 1, 5, False), (4, 7, 1, False)] + [(4, m, m, False) for m in (P - 1, P, P + 1)] + [(4, 9 * P + 1, 9 * P + 1, True)]
    if d >= 32:
        own = sorted({wide_points(g, 8), 16 if d == 128 else wide_points(g, 8)})        # statistics kernel; the d = 128 parameter pass
        cases += [(16, 1, 17, True), (16, 7, 1, True)] + [(16, w + o, w + o, True) for w in own for o in (-1, 0, 1)]
    return cases


@pytest.mark.parametrize('d', WIDTHS)
def test_row_counts(d):
    """K = 4, m = 1 (bipartite both ways: one target over K + 1 sources, seven targets over one source), PPB - 1, PPB, PPB + 1 and
    9 PPB + 1 (ten workgroups: not a multiple of the 8 XCDs my_row_at remaps over; the last holds one row; also deferred).  The lanes past
    m are clamped onto row m - 1 and masked by `live`: a double-counted row is a large part of every sum here.  At d >= 32 also K = 16:
    m = 1 both ways and one under, at and one over the points per workgroup of the matrix-pipe statistics kernel (8 below 2048 targets) and
    of the d = 128 parameter pass (16), immediate and deferred.  Bounds and CPU e32: BOUNDS['rows']."""
    g = geometry(d)
    assert nblocks(g, 9 * g['PPB'] + 1) == 10 and 10 % 8 != 0
    for K, m_tgt, m_src, df in row_count_cases(d):
        rng = seed(3, d, K, m_tgt, m_src)
        if m_tgt == m_src:
            tab = self_table(self_rows(rng, m_tgt, K))
        elif m_tgt == 1:
            tab = bipartite_rows(np.arange(K)[None], K + 1)                  # K distinct sources, one more without an in-edge
        else:
            tab = bipartite_rows(np.zeros((7, K), dtype=np.int64), 1)        # seven targets, all entries the one source
        inp = pc_inputs(rng, m_src, m_tgt, d, m_tgt != m_src)
        pc_check('rows', inp, tab, True, (False, True) if df else (False,))


# ------------------------------------------------------------------ 4: how the statistics are finished
def finish_cases(d):
    """(K, m, what the case is for) of test_statistics_finish at width d."""
    g = geometry(d)
    P, R = g['PPB'], g['RPI'] * g['RED_TRIPS']
    cases = [(2 if d <= 8 else 4, (n - 1) * P + 1, 'scalar %d' % n) for n in (g['LW_FLAT'] + 1, 80, 97)]
    if d >= 64:
        n = g['NT'] // (d // 2) + 1
        cases.append((2, (n - 1) * P + 1, 'scalar %d none' % n))
    if d >= 32:
        cases.append((16, g['LW_FLAT'] * wide_points(g, 8) + 9, 'mfma %d' % (g['LW_FLAT'] + 2)))
    cases += [(4, R - 1, 'reduce 1'), (4, R + 3, 'reduce 2')]
    if d == 128:
        cases.append((2, g['LW_FLAT'] * R + 1, 'reduce %d' % (g['LW_FLAT'] + 1)))
    return cases


@pytest.mark.parametrize('d', WIDTHS)
def test_statistics_finish(d):
    """crfconv_pointconv_forward_uv finishes the BatchNorm-2 statistics by a flat ticket up to LW_FLAT = 64 workgroups (every other
    test), by a two-level ticket above (here 65, 80 and 97 workgroups: 65 % 32 = 97 % 32 = 1 -- one group of LW_GROUPS = 32 larger than
    the others --, 80 % 32 = 16), and without a ticket by a reduce_partials launch when nblk (d / 2) > 256 * 24: 193 workgroups at
    d = 64, 97 at d = 128 (m = 769 and 385).  The last workgroup holds one row.  K = 16 at d >= 32: 66 workgroups of the matrix-pipe
    statistics kernel (two-level).  uv_bwd_reduce_body, riding in the input-gradient launch: 1 and 2 reduce workgroups, at d = 128 also
    65 (two-level ticket of its own), with odd and even numbers of row trips per thread (the two-rows-in-flight loop and its tail).
    Every property is asserted from `geometry`.  Bounds and CPU e32: BOUNDS['finish']."""
    g = geometry(d)
    seen, trips = set(), set()
    for K, m, what in finish_cases(d):
        kernel, n, finish = stats_finish(g, d, K, m)
        kind, count = what.split()[0], int(what.split()[1])
        if kind == 'scalar':
            assert kernel == 'scalar' and n == count > g['LW_FLAT'] and (m - 1) % g['PPB'] == 0
            if what.endswith('none'):                                  # the smallest count past the rule
                assert finish == 'none' and (n - 1) * (d // 2) <= g['NT']
            seen.add((finish, n % g['LW_GROUPS']))
        elif kind == 'mfma':
            assert kernel == 'mfma' and n == count > g['LW_FLAT'] and finish == 'two-level'
        else:
            assert reduce_blocks(g, m) == count
        trips |= reduce_trips(g, m)
        rng = seed(4, d, K, m)
        tab = self_table(self_rows(rng, m, K))
        pc_check('finish', pc_inputs(rng, m, m, d, False), tab, True)
    assert any(v % 2 == 1 for v in trips) and any(v % 2 == 0 and v > 0 for v in trips), trips
    assert {('two-level', 1), ('two-level', 16)} <= seen and any(f == 'none' for f, _ in seen) == (d >= 64), seen


# ------------------------------------------------------------------ 5: padded and bipartite tables
@pytest.mark.parametrize('K,train', [(7, True), (7, False), (16, True)])
@pytest.mark.parametrize('d', WIDTHS)
def test_padded_and_bipartite(d, K, train):
    """graph.table_from_edges from a SHUFFLED edge list over 451 sources and 700 targets: entries per target drawn from {0, 1, 3, K}, source
    0 a hub of in-degree >= 200 (bwd_input_kernel walks to the wavefront's largest in-degree), eight sources without an in-edge (dx rows
    exactly 0), the last target without an entry (out row exactly 0); n_edges is the valid count and both BatchNorms' statistics are over
    the valid edges only.  K = 7: eid / K instead of a shift in the reverse walk, train and eval; K = 16: the matrix-pipe kernels over
    holes, immediate and deferred.  All asserted on the table read back (`ragged_table`).  Bounds and CPU e32: BOUNDS['padded']."""
    m_tgt, m_src = 700, 451
    rng = seed(5, d, K, train)
    tab = ragged_table(rng, m_tgt, m_src, K)
    inp = pc_inputs(rng, m_src, m_tgt, d, True)
    rows, _ = pc_check('padded', inp, tab, train, (False, True) if K == 16 else (False,))
    assert int((~(rows >= 0).any(1)).sum()) >= 2


# ------------------------------------------------------------------ 6: input regimes
@pytest.mark.parametrize('K', [6, 16])
@pytest.mark.parametrize('d', [8, 32, 128])
def test_input_regimes(d, K):
    """The sparse twin's regime: slope 0.01; gout of order 1e-5 with column means near 0 (a mean cross-entropy over 10^5 points); x with
    a mean of 3; positions in a box centred at 50 with neighbour distances of ~0.05 (scene coordinates: rel is a small difference of large
    float32 numbers; the reference takes the float32 positions as given).  Dense self table, m = 2 PPB + 3 rows of a jittered chain, training,
    immediate and deferred.  Bounds and CPU e32: BOUNDS['regime']."""
    g = geometry(d)
    m = max(2 * g['PPB'] + 3, 67)
    rng = seed(6, d, K)
    rows = (np.arange(m)[:, None] + rng.integers(-8, 9, (m, K))) % m              # neighbours along the chain
    rows[:, 0] = np.arange(m)
    inp = pc_inputs(rng, m, m, d, False, slope=0.01)
    chain = np.stack([50.0 + 0.01 * np.arange(m), 50.0 + 0.02 * np.sin(np.arange(m)), np.full(m, 50.0)], 1)
    inp['ps'] = inp['pt'] = torch.from_numpy((chain + 0.01 * rng.standard_normal((m, 3))).astype(np.float32))
    inp['x'] = inp['x'] + 3.0
    gout = rng.standard_normal((m, d))
    inp['gout'] = torch.from_numpy((1e-5 * (gout - gout.mean(0))).astype(np.float32))
    tab = self_table(rows)
    rel = inp['pt'][:, None, :] - inp['ps'][device_rows(tab)]
    assert 0.02 < float(rel.norm(dim=-1)[:, 1:].median()) < 0.1 and float(inp['gout'].mean(0).abs().max()) < 1e-11
    pc_check('regime', inp, tab, True, (False, True))


# ------------------------------------------------------------------ 7: the moments and the running statistics, as tensors of their own
@pytest.mark.parametrize('kind', ['dense', 'padded', 'bipartite'])
@pytest.mark.parametrize('d', [8, 64])
def test_moments_and_running_statistics(d, kind):
    """ops.relpos_moments (mean [3], covariance [3, 3]) and the four running tensors after ONE training forward from running statistics of
    ZERO, so that each is 0.1 x the batch statistic on its own scale (from the default (0, 1) the running variance would hide a wrong
    batch variance behind 0.9): fold1 publishes BatchNorm-1's from the moments (mean W1 mean_rel, variance diag(W1 cov W1^T) n / (n - 1)),
    uv_publish BatchNorm-2's from the edge pass.  dense: self table, m = 300, K = 5; padded: table_from_edges over 300 rows, entries per
    target from {0, 1, 3, 7} (valid edges only);
    bipartite: 40 targets over 9 sources, K = 3 (n = 120: n / (n - 1) is 0.8 % of the variance).  Bounds and CPU e32: BOUNDS['moments']."""
    rng = seed(7, d, len(kind))
    if kind == 'dense':
        m_tgt = m_src = 300
        tab = self_table(self_rows(rng, 300, 5))
    elif kind == 'padded':
        m_tgt = m_src = 300
        tab = edges_table(rng, 300, (0, 1, 3, 7))
    else:
        m_tgt, m_src = 40, 9
        tab = bipartite_rows(rng.integers(0, m_src, (m_tgt, 3)), m_src)
    inp = pc_inputs(rng, m_src, m_tgt, d, kind != 'dense')
    for k in RUNNING:
        inp[k] = torch.zeros(d)
    pc_check('moments', inp, tab, True, only=('mean', 'cov') + RUNNING)


# ------------------------------------------------------------------ 8: holes anywhere in a row
@pytest.mark.parametrize('d', WIDTHS)
def test_holes_anywhere(d):
    """graph.table_from_index with -1 entries ANYWHERE in a row (what a radius-limited search leaves; table_from_edges packs a row's
    entries to the left, so tests 5 and 7 never put a hole in front of an entry): test_gpu_discrete's 'ragged' rows at K = 9, m = 151 --
    35 % holes in leading and interior columns (inside an EB batch, inside a UV_GROUP trip), two hub sources, repeated sources, self
    edges, three rows without an entry -- with n_edges set to the valid count, as the table builders do.  Training, immediate and deferred,
    and eval.  Bounds and CPU e32: BOUNDS['holes']."""
    m, K = 151, 9
    for train in (True, False):
        rng = seed(8, d, train)
        tab = index_table(shaped_rows('ragged', rng, m, K))
        rows = device_rows(tab)
        tab.n_edges = int((rows >= 0).sum())
        inner = (rows[:, :-1] < 0) & (rows[:, 1:] >= 0)                # a hole directly in front of an entry
        assert tab.padded and int(inner.any(1).sum()) > m // 2 and int((~(rows >= 0).any(1)).sum()) == 3
        pc_check('holes', pc_inputs(rng, m, m, d, False), tab, train, (False, True))
