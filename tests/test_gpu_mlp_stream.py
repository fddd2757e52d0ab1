"""-m gpu: the row-streaming dense stack of the fine levels, form by form, against a float64 reference written here in plain torch with
autograd on the CPU -- linear_fwd_kernel in every instantiation lf_launch can reach (csrc/linear_fwd.hpp, linear.hip: forward, the
transposed dX product, dropout mask, two-pointer operand, eval-mode BatchNorm epilogue; csrc/mlp_bwd.hip: the PRO = true dX forms with
the addend and the masked epilogue), BatchNorm from the product's statistic records (csrc/bn_records.hip), the fused backward's first
pass in its eight tile classes with and without the last-workgroup ticket, its finalize (csrc/mlp_bwd.hip), and the weight gradient of
the plain product (csrc/wgrad.hip, wgrad_body.hpp).

Forcing the family: the fixture `streaming` sets ops.state.mfma_min_rows = 1, so _mlp_small_ok is false for every m and ops.linear,
ops.mlp_block, _join, _cat, _dropout, ops.mlp_dropout_linear and ops.linear_bn_act take the row-streaming kernels at every row count.
Each case asserts the autograd node it expects and which library entries ran (test_gpu_pointconv's `recorded`).

The reference (`block_reference`) restates y = x W^T (+ b), the training BatchNorm (biased batch statistics; running statistics with
momentum 0.1 and the unbiased n / (n - 1)), + skip, LeakyReLU, dropout (the mask of ops.dropout_keep_mask with the node's seed and
counter, scaled by 1 / (1 - p)) and the Linear behind it.  It runs once in float64 and once in float32 and returns out, the input
gradients, dW, dgamma, dbeta, db, the running tensors (for ops.linear: y, and the mean / rstd that crfconv_bn_coef_from_records forms
from the statistic records).  Products over the row dimension are formed in 64-row blocks (test_gpu_pointconv.rows_matmul), so the
float32 run does not depend on a BLAS's summation order.

The LeakyReLU kink, by construction: no branch is taken from the kernel.  `nudge` moves beta of every channel whose float64
pre-activation (+ skip for a join) comes within TAU = 1e-4 of 0, by the nearest shift that leaves none within TAU (as
test_gpu_pointconv.nudge_beta1), and every case asserts min |pre| >= TAU over all rows and channels.  For the masked dX epilogue the mask
reference is the join's output: the case runs the public chain mlp_block_join(..., mask=hs) -> mlp_block(..., fork=True, input_mask=hs)
and both betas are nudged, the join's first.  No channel is left out of any comparison.

The comparison is test_gpu_discrete's `own_scale` on every tensor's OWN scale: e = max|got - ref64| / max|ref64| <= max(bound, 4 e32),
and e32 <= bound is asserted too.  A bound belongs to a (site, tensor) pair (BOUNDS): 10 x the largest e32 the float32 restatement
showed on the CPU over the site's cases (another summation order), rounded up to one digit, never below 1e-6.  `python
tests/test_gpu_mlp_stream.py` runs the restatements of every case without a GPU and prints that column.  Inputs: x with a mean of 0.5,
W ~ N(0, 1) / sqrt(Ci), gamma in 0.5 .. 1.5, upstream gradients 0.3 + 0.5 N(0, 1) (except in block_regimes).  No compared tensor is zero
by cancellation alone: `prepare` asserts that max|ref64| of every tensor is above 1e-3 of the largest of its case and kind (KINDS:
per-row forward values, means, variances, per-row gradients and sums over the rows, each among themselves -- the regime with an upstream
gradient of 1e-5 scales every gradient and a sum over the rows grows with the row count, so no figure across kinds or cases means
anything).  Structural zeros -- the dropped elements of a dropout block's output -- are exact zeros.  Before every forward and backward
the allocator is poisoned with NaN blocks of the outputs' shapes, and for every case the rule must refuse each tensor zeroed and
mis-scaled by 10 x its bound.

The kernels' geometry is READ from the sources (`geometry`): constants by name, the formulas of lf_tco, lf_lds_bytes_at,
lf_hoist_chunks, lf_blocks, lf_form, mlp_plan (with the tco * tci == 16 -> tci = 2 rule), the ticket rule, wg_plan, bn_apply_plan and
LASTWG_FLAT_ restated beside regular expressions over the text they restate.  Each case asserts the property it is named for, and
test_every_form_is_reached asserts that the union of the cases reaches every (TCO, VEC4, NCH, EPI, PRO) for which lf_form is true, except
EPI_UV, and every (tco, tci) class of mlp_plan's switch.

Not here, and held today by: the coarse family mlp_small*.hip / gemm_stats.hip / _MLPSmall* (test_gpu_mlp_small.py, form by form against
the same reference; its UV operand forms, the eval epilogue and the plain product: test_gpu_operand_fold.py, test_gpu_infer.py,
test_gpu_model.py), head.hip / _HeadRecompute (test_gpu_model.py, test_gpu_mlp_nodes.py), mlp_block_pool
(test_gpu_pool.py, test_gpu_mlp_nodes.py), the EPI_UV operand fold (test_gpu_operand_fold.py), deferred delivery (test_gpu_mlp_nodes.py,
test_gpu_backward_tail.py), the stand-alone statistics pass of bn.hip (test_gpu_model.py, test_gpu_infer.py) and loss.hip
(test_gpu_model.py, test_gpu_native.py).  Measured figures per site: BOUNDS and
profiles/r28_mlp_float64.md."""
import contextlib
import functools
import os
import re
import sys
import zlib

import numpy as np
import pytest
import torch

if __name__ == '__main__':                                     # the CPU column of BOUNDS: no pytest, no GPU
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_util import DEV
from test_gpu_discrete import dev, errors, leaf, own_scale, poison, rejected
from test_gpu_pointconv import _csrc_int, _src, recorded, rows_matmul, seed

pytestmark = pytest.mark.gpu

TAU, EPS, MOM = 1e-4, 1e-5, 0.1
EPI_NONE, EPI_ADD, EPI_DROPOUT, EPI_ADD_MASK, EPI_UV, EPI_BN_ACT = range(6)
# tensors whose sizes can be set against each other: per-row forward values, means, variances, per-row gradients; every other tensor is
# a sum over the rows
KINDS = (('out', 'j_out'), ('rm', 'j_rm', 'mean'), ('rv', 'j_rv', 'rstd'), ('dx', 'dxb', 'dskip'))

# site -> tensor -> (bound, largest e32 of the float32 restatement on the CPU, largest e measured on the MI355X).  bound = 10 x the e32 of
# the CPU run made BEFORE the GPU run, rounded up to one digit, never below 1e-6 = 16 float32 roundings; the e32 recorded here is the
# larger of that run's and of the restatement on the MI355X machine's host CPU (profiles/r28_mlp_float64.md lists both).  site/sub: a few
# cases of a site that are conditioned unlike the others (`case`).
BOUNDS = {
    'linear_forms': dict(out=(6e-06, 5.8e-07, 8.5e-07), dx=(7e-06, 6.8e-07, 4.9e-07), dW=(3e-06, 2.3e-07, 1.8e-07), db=(2e-06, 1.7e-07, 1.1e-07)),
    'linear_rows': dict(mean=(2e-06, 1.9e-07, 1.8e-07), rstd=(2e-06, 1.5e-07, 3.4e-07), out=(4e-06, 3.7e-07, 3.3e-07), dx=(5e-06, 4.0e-07, 3.5e-07),
                        dW=(4e-06, 3.3e-07, 1.7e-07), db=(2e-06, 1.1e-07, 9.0e-08)),
    'block_widths': dict(rm=(2e-06, 1.2e-07, 7.7e-08), rv=(1e-06, 1.0e-07, 5.0e-08), out=(6e-06, 5.0e-07, 5.1e-07), dx=(6e-06, 5.1e-07, 5.5e-07),
                         dW=(7e-06, 6.2e-07, 4.4e-07), dgamma=(8e-06, 7.9e-07, 4.7e-07), dbeta=(2e-06, 1.8e-07, 8.3e-08)),
    'block_rows/2': dict(rm=(2e-06, 1.1e-07, 8.6e-08), rv=(1e-06, 9.9e-08, 7.9e-08), out=(2e-05, 1.0e-06, 1.1e-06), dx=(2e-03, 1.1e-04, 1.1e-04),
                         dW=(2e-03, 1.7e-04, 1.8e-04), dgamma=(7e-06, 6.9e-07, 6.5e-07), dbeta=(1e-06, 4.2e-08, 4.2e-08)),
    'block_rows': dict(rm=(2e-06, 1.3e-07, 7.6e-08), rv=(1e-06, 9.7e-08, 1.1e-07), out=(4e-06, 3.0e-07, 4.2e-07), dx=(4e-06, 3.7e-07, 3.7e-07),
                       dW=(3e-05, 2.8e-06, 1.6e-06), dgamma=(4e-06, 3.2e-07, 4.3e-07), dbeta=(2e-06, 1.4e-07, 1.1e-07)),
    'fork_and_mask': dict(rm=(2e-06, 1.2e-07, 6.9e-08), rv=(2e-06, 1.0e-07, 6.2e-08), out=(4e-06, 4.5e-07, 3.5e-07), dx=(5e-06, 4.9e-07, 3.8e-07),
                          dW=(6e-06, 6.7e-07, 6.8e-07), dgamma=(3e-06, 2.7e-07, 2.7e-07), dbeta=(2e-06, 1.5e-07, 1.1e-07),
                          j_rm=(2e-06, 1.1e-07, 7.2e-08), j_rv=(2e-06, 1.0e-07, 5.7e-08), j_out=(3e-06, 2.5e-07, 2.0e-07),
                          j_dW=(5e-06, 6.9e-07, 4.4e-07), dskip=(6e-06, 6.5e-07, 4.5e-07), j_dgamma=(6e-06, 6.2e-07, 5.4e-07),
                          j_dbeta=(2e-05, 1.4e-06, 9.6e-07)),
    'join': dict(rm=(2e-06, 1.3e-07, 3.9e-08), rv=(1e-06, 7.7e-08, 5.1e-08), out=(3e-06, 2.4e-07, 1.8e-07), dx=(4e-06, 3.3e-07, 3.5e-07),
                 dW=(7e-06, 6.2e-07, 3.3e-07), dskip=(1e-06, 4.5e-09, 4.5e-09), dgamma=(2e-06, 1.9e-07, 1.8e-07), dbeta=(2e-06, 1.2e-07, 6.5e-08)),
    'cat': dict(rm=(1e-06, 8.6e-08, 5.0e-08), rv=(1e-06, 9.5e-08, 4.3e-08), out=(5e-06, 4.6e-07, 3.9e-07), dx=(3e-06, 2.8e-07, 4.0e-07),
                dxb=(3e-06, 2.6e-07, 2.9e-07), dW=(3e-06, 3.6e-07, 2.9e-07), dgamma=(3e-06, 2.1e-07, 1.7e-07), dbeta=(2e-06, 1.3e-07, 6.2e-08)),
    'dropout': dict(rm=(2e-06, 1.2e-07, 5.0e-08), rv=(1e-06, 9.9e-08, 4.7e-08), out=(4e-06, 3.4e-07, 3.6e-07), dx=(5e-06, 4.4e-07, 7.0e-07),
                    dW=(9e-06, 8.7e-07, 6.2e-07), dgamma=(4e-06, 3.0e-07, 1.6e-07), dbeta=(2e-06, 1.5e-07, 1.3e-07), dW2=(2e-06, 2.2e-07, 1.7e-07),
                    db2=(2e-06, 1.2e-07, 1.1e-07)),
    'eval': dict(out=(5e-06, 4.4e-07, 5.2e-07)),
    'block_regimes/shifted': dict(rm=(3e-06, 2.0e-07, 3.7e-08), rv=(5e-06, 4.8e-07, 2.9e-07), out=(3e-04, 3.0e-05, 2.4e-05),
                                  dx=(9e-05, 8.5e-06, 4.2e-06), dW=(9e-02, 8.3e-03, 1.8e-03), dgamma=(8e-04, 7.5e-05, 1.6e-05),
                                  dbeta=(2e-06, 1.1e-07, 6.5e-08)),
    'block_regimes/small gradient': dict(rm=(1e-06, 8.9e-08, 3.7e-08), rv=(1e-06, 8.6e-08, 4.4e-08), out=(3e-06, 2.7e-07, 2.4e-07),
                                         dx=(4e-06, 3.0e-07, 3.4e-07), dW=(2e-06, 1.9e-07, 1.5e-07), dgamma=(3e-06, 2.3e-07, 1.9e-07),
                                         dbeta=(2e-06, 1.3e-07, 1.1e-07)),
    'block_regimes/constant column': dict(rm=(2e-06, 1.2e-07, 4.5e-08), rv=(1e-06, 7.7e-08, 4.4e-08), out=(8e-04, 7.5e-05, 8.2e-05),
                                          dx=(1e-04, 9.9e-06, 7.8e-06), dW=(4e-04, 3.2e-05, 1.6e-05), dgamma=(2e-03, 1.0e-04, 2.4e-05),
                                          dbeta=(2e-06, 1.2e-07, 5.4e-08)),
}


def bound(site, name):
    return BOUNDS[site][name][0]


# ------------------------------------------------------------------ the kernels' geometry, read from the sources
@functools.lru_cache(maxsize=None)
def constants():
    """The tunables the plans depend on, by name, after checking the text of every formula `geometry` restates."""
    fwd, bwd, wg, bnr = _src('linear_fwd.hpp'), _src('mlp_bwd.hip'), _src('wgrad_body.hpp'), _src('bn_records.hip')

    def need(text, *patterns):
        for p in patterns:
            assert re.search(p, text), 'the sources no longer say: %s' % p

    def num(text, pattern):
        hit = re.search(pattern, text)
        assert hit, 'the sources no longer say: %s' % pattern
        return int(hit.group(1))
    k = dict(LF_BLOCK=_csrc_int('linear_fwd.hpp', 'LF_BLOCK_'), PF_MAX=_csrc_int('linear_fwd.hpp', 'LF_PF_MAX_'),
             WG_BLOCK=_csrc_int('wgrad_body.hpp', 'WG_BLOCK'), LW_FLAT=_csrc_int('gridsync.hpp', 'LASTWG_FLAT_'),
             P1_TARGET=_csrc_int('mlp_bwd.hip', 'MLP_P1_TARGET_'), WG_LONG=_csrc_int('wgrad_body.hpp', 'WG_LONG_ROWS_'),
             BN_WGS=_csrc_int('bn_records.hip', 'BN_APPLY_WGS_'), FR_CH=num(bnr, r'constexpr int FR_BLOCK = 1024, FR_CH = (\d+),'),
             BA_MAX=_csrc_int('bn_records.hip', 'BA_MAX'))
    need(fwd, r'constexpr int EPI_NONE = 0, EPI_ADD = 1, EPI_DROPOUT = 2, EPI_ADD_MASK = 3, EPI_UV = 4, EPI_BN_ACT = 5;',
         r'constexpr int LF_BLOCK = LF_BLOCK_, LF_WAVES = LF_BLOCK / WAVE;', r'constexpr bool PF = NCH > 0 && NCH <= LF_PF_MAX_;')
    # lf_blocks
    k['CAP'] = num(fwd, r'static int lf_blocks\(int64_t M\) \{\s*constexpr int cap = (\d+);')
    need(fwd, r'int64_t nb = \(M \+ 16 \* LF_WAVES - 1\) / \(16 \* LF_WAVES\);', r'if \(nb > cap\) nb = cap;', r'return \(int\)\(nb < 1 \? 1 : nb\);')
    # lf_lds_bytes_at
    need(fwd, r'const size_t cip = \(size_t\)\(\(Ci \+ 15\) / 16\) \* 16 \+ 4, cik = cip - 4;', r'size_t floats = 16 \* \(size_t\)tco \* cip;',
         r'const size_t stats = \(size_t\)crf::LF_WAVES \* 4 \* 16 \* \(size_t\)tco;', r'if \(floats < stats\) floats = stats;',
         r'if \(pro\) floats \+= 5 \* cik;', r'if \(tco >= 2\) floats \+= \(size_t\)crf::LF_WAVES \* 16 \* \(16 \* \(size_t\)tco \+ 4\);')
    # lf_tco
    k['MAX_TCO'] = num(fwd, r'constexpr int max_tco = (\d+);')
    need(fwd, r'int tco = tiles >= max_tco \? max_tco : \(tiles >= 2 \? 2 : 1\);',
         r'while \(tco > 1 && lf_lds_bytes_at\(Ci, tco, pro\) > 64 \* 1024\) tco >>= 1;')
    # lf_hoist_chunks, lf_launch
    need(fwd, r'if \(!vec4 \|\| Ci > 128\) return 0;', r'return n <= 1 \? 1 : \(n <= 2 \? 2 : \(n <= 4 \? 4 : 8\)\);',
         r'const bool vec4 = \(a\.Ci % 4\) == 0 && \(a\.Co % 4\) == 0;', r'const int nch = epi == EPI_DROPOUT \? 0 : lf_hoist_chunks\(a\.Ci, vec4\);',
         r'const dim3 grid\(\(unsigned\)lf_blocks\(a\.M\), \(unsigned\)\(\(tiles \+ tco - 1\) / tco\)\)',
         r'lf_pick<1, 2, 4>\(tco,', r'lf_pick<0, 1>\(vec4,', r'lf_pick<0, 1, 2, 4, 8>\(nch,')
    # lf_form
    need(fwd, r'if \(EPI == EPI_UV\) return !PRO && VEC4 && TCO >= 2 && NCH == 1;',
         r'if \(NCH > 0 && \(!VEC4 \|\| EPI == EPI_DROPOUT\)\) return false;',
         r'if \(PRO\) return EPI == EPI_NONE \|\| EPI == EPI_ADD \|\| \(EPI == EPI_ADD_MASK && VEC4\);',
         r'return EPI == EPI_NONE \|\| EPI == EPI_DROPOUT \|\| EPI == EPI_BN_ACT;')
    # mlp_plan, the ticket rule, the classes of its switch
    need(bwd, r'p\.tco = t_co >= 4 \? 4 : \(t_co >= 2 \? 2 : 1\);', r'p\.tci = t_ci >= 4 \? 4 : \(t_ci >= 2 \? 2 : 1\);',
         r'if \(p\.tco \* p\.tci == 16\) p\.tci = 2;', r'p\.gy = \(t_co \+ p\.tco - 1\) / p\.tco;', r'p\.gz = \(t_ci \+ p\.tci - 1\) / p\.tci;',
         r'int64_t slices = target / \(\(int64_t\)p\.gy \* p\.gz\);\s*if \(slices < 32\) slices = 32;',
         r'int64_t rows = \(M \+ slices - 1\) / slices;\s*if \(rows < 64\) rows = 64;\s*rows = \(rows \+ 63\) / 64 \* 64;',
         r'p\.nblk = \(int\)\(\(M \+ rows - 1\) / rows\);',
         r'if \(!\(2 \* Co <= crf::WG_BLOCK && crf::WG_BLOCK % \(Co / 2\) == 0 && ',
         r'last_workgroup\(ticket, gridDim\.x \* gridDim\.y \* gridDim\.z, &s_flag\)')
    k['P1'] = frozenset((int(a), int(b)) for a, b in re.findall(r'(?:case \d\d|default): P1\((\d), (\d)\); break;', bwd))
    assert len(k['P1']) == 8, k['P1']
    need(_src('gridsync.hpp'), r'if \(nblk <= LW_FLAT\) \{')
    # wg_plan
    need(wg, r'int64_t slices = 512 / \(\(int64_t\)p\.gy \* p\.gz\);\s*if \(slices < 32\) slices = 32;', r'if \(M <= 65536\) \{',
         r'int64_t want = WG_LONG_ROWS_;\s*if \(M < 2 \* want\) want = \(\(M \+ 1\) / 2 \+ 63\) / 64 \* 64;\s*if \(rows < want\) rows = want;')
    # bn_apply_plan
    need(bnr, r'const int slabs = \(C \+ crf::FR_CH - 1\) / crf::FR_CH;\s*tiles = wgs / slabs;\s*if \(tiles < 1\) tiles = 1;',
         r'rows = \(M \+ tiles - 1\) / tiles;\s*rows = \(rows \+ 1023\) / 1024 \* 1024;\s*tiles = \(M \+ rows - 1\) / rows;',
         r'if \(tiles > 8\) tiles = \(tiles \+ 7\) / 8 \* 8;', r'bn_apply_plan\(M, C, BN_APPLY_WGS_, tiles, rows\);')
    return k


def cdiv(a, b):
    return -(-a // b)


def lf_lds_bytes_at(ci, tco, pro):
    waves = constants()['LF_BLOCK'] // 64
    cip = cdiv(ci, 16) * 16 + 4
    floats = max(16 * tco * cip, waves * 4 * 16 * tco) + (5 * (cip - 4) if pro else 0) + (waves * 16 * (16 * tco + 4) if tco >= 2 else 0)
    return 4 * floats


def lf_tco(ci, co, pro):
    tiles, top = cdiv(co, 16), constants()['MAX_TCO']
    tco = top if tiles >= top else (2 if tiles >= 2 else 1)
    while tco > 1 and lf_lds_bytes_at(ci, tco, pro) > 64 * 1024:
        tco >>= 1
    return tco


def lf_hoist_chunks(ci, vec4):
    if not vec4 or ci > 128:
        return 0
    n = cdiv(ci, 16)
    return 1 if n <= 1 else (2 if n <= 2 else (4 if n <= 4 else 8))


def lf_blocks(m):
    return max(1, min(cdiv(m, 16 * (constants()['LF_BLOCK'] // 64)), constants()['CAP']))


def lf_form(tco, pro, vec4, epi, nch):
    if epi == EPI_UV:
        return not pro and vec4 and tco >= 2 and nch == 1
    if nch > 0 and (not vec4 or epi == EPI_DROPOUT):
        return False
    if pro:
        return epi in (EPI_NONE, EPI_ADD) or (epi == EPI_ADD_MASK and vec4)
    return epi in (EPI_NONE, EPI_DROPOUT, EPI_BN_ACT)


def tile_plan(m, co, ci, target, long_rows):
    """mlp_plan (long_rows = 0) and wg_plan of the sources: (tco, tci, gy, gz, nblk, rows_per_block)."""
    t_co, t_ci = cdiv(co, 16), cdiv(ci, 16)
    tco = 4 if t_co >= 4 else (2 if t_co >= 2 else 1)
    tci = 4 if t_ci >= 4 else (2 if t_ci >= 2 else 1)
    if not long_rows and tco * tci == 16:
        tci = 2
    gy, gz = cdiv(t_co, tco), cdiv(t_ci, tci)
    rows = cdiv(max(cdiv(m, max(target // (gy * gz), 32)), 64), 64) * 64
    if long_rows > 64 and m <= 65536:
        want = long_rows if m >= 2 * long_rows else cdiv((m + 1) // 2, 64) * 64
        rows = max(rows, want)
    return dict(tco=tco, tci=tci, gy=gy, gz=gz, nblk=cdiv(m, rows), rows=rows)


def bn_apply_plan(m, c):
    k = constants()
    tiles = max(k['BN_WGS'] // cdiv(c, k['FR_CH']), 1)
    rows = cdiv(cdiv(m, tiles), 1024) * 1024
    tiles = cdiv(m, rows)
    live = tiles
    if tiles > 8:
        tiles = cdiv(tiles, 8) * 8
    return dict(tiles=tiles, live=live, rows=rows, slabs=cdiv(c, k['FR_CH']))


def geometry(ci, co, m, pro):
    """Plans of a layer x [m, ci] -> y [m, co].  'lf': the linear_fwd_kernel launch -- pro False: the forward product (ci inputs, co
    outputs); pro True: the dX product of the fused backward (co inputs, ci outputs, PRO) -- as (tco, vec4, nch) with its grid, LDS bytes
    and whether the loop prefetches (pf) and how many row groups a wavefront takes at most and at least (groups).  'p1': mlp_plan of
    the fused backward's first pass, 'ticket': whether its last workgroup does the channel part and in how many levels it draws, 'wg':
    wg_plan of the plain weight gradient, 'bn': bn_apply_plan of the apply launch."""
    k = constants()
    kin, nout = (co, ci) if pro else (ci, co)
    tco, vec4 = lf_tco(kin, nout, pro), kin % 4 == 0 and nout % 4 == 0
    nch = lf_hoist_chunks(kin, vec4)
    gx = lf_blocks(m)
    waves = gx * (k['LF_BLOCK'] // 64)
    lf = dict(tco=tco, vec4=vec4, nch=nch, pf=0 < nch <= k['PF_MAX'], gx=gx, gy=cdiv(cdiv(nout, 16), tco), lds=lf_lds_bytes_at(kin, tco, pro),
              groups=(cdiv(cdiv(m, 16), waves), cdiv(m, 16) // waves), fits=lf_lds_bytes_at(kin, lf_tco(kin, nout, pro), pro) <= 64 * 1024)
    p1 = tile_plan(m, co, ci, k['P1_TARGET'], 0)
    grid = p1['nblk'] * p1['gy'] * p1['gz']
    ticket = co % 4 == 0 and 2 * co <= k['WG_BLOCK'] and k['WG_BLOCK'] % (co // 2) == 0
    return dict(lf=lf, p1=p1, ticket=('flat' if grid <= k['LW_FLAT'] else 'two-level') if ticket else 'none', p1_grid=grid,
                wg=tile_plan(m, co, ci, 512, k['WG_LONG']), bn=bn_apply_plan(m, co))


def form(kin, nout, pro, epi):
    """The instantiation (TCO, VEC4, NCH, EPI, PRO) lf_launch picks for kin inputs and nout outputs."""
    vec4 = kin % 4 == 0 and nout % 4 == 0
    f = (lf_tco(kin, nout, pro), int(vec4), 0 if epi == EPI_DROPOUT else lf_hoist_chunks(kin, vec4), epi, int(pro))
    assert lf_form(f[0], pro, vec4, epi, f[2]), f
    return f


def every_form():
    return {(tco, vec4, nch, epi, pro) for tco in (1, 2, 4) for vec4 in (0, 1) for nch in (0, 1, 2, 4, 8) for pro in (0, 1)
            for epi in (EPI_NONE, EPI_ADD, EPI_DROPOUT, EPI_ADD_MASK, EPI_BN_ACT) if lf_form(tco, bool(pro), bool(vec4), epi, nch)}


# ------------------------------------------------------------------ float64 / float32 reference (plain torch, autograd)
GRAD_NAMES = {'x': 'dx', 'xb': 'dxb', 'W': 'dW', 'bias': 'db', 'g': 'dgamma', 'b': 'dbeta', 'skip': 'dskip', 'W2': 'dW2', 'b2': 'db2',
              'j_W': 'j_dW', 'j_g': 'j_dgamma', 'j_b': 'j_dbeta'}


def lrelu(v, slope):
    return torch.where(v > 0, v, slope * v)


def _forward(inp, dtype, grad):
    """(results, leaves, [(prefix, pre-activation)]) of a case's forward in `dtype`; grad: the inputs are fresh autograd leaves."""
    leaves, res, pres = {}, {}, []
    kind = inp['kind']

    def L(k):
        if k not in leaves:
            leaves[k] = leaf(inp[k], dtype) if grad else inp[k].to(dtype)
        return leaves[k]

    def bn(y, pfx, skip):
        mu, var = y.mean(0), y.var(0, unbiased=False)
        pre = (y - mu) / torch.sqrt(var + EPS) * L(pfx + 'g') + L(pfx + 'b')
        if skip is not None:
            pre = pre + skip
        n = y.shape[0]
        res[pfx + 'rm'] = ((1.0 - MOM) * inp[pfx + 'rm'].to(dtype) + MOM * mu).detach()
        res[pfx + 'rv'] = ((1.0 - MOM) * inp[pfx + 'rv'].to(dtype) + MOM * var * (n / (n - 1.0))).detach()
        pres.append((pfx, pre.detach()))
        return pre
    h = L('x')
    if kind == 'chain':
        h = lrelu(bn(rows_matmul(h, L('j_W').t()), 'j_', L('skip')), inp['j_slope'])
        res['j_out'] = h
    elif 'xb' in inp:
        h = torch.cat([h, L('xb')], 1)
    y = rows_matmul(h, L('W').t())
    if 'bias' in inp:
        y = y + L('bias')
    out = y
    if kind == 'eval':
        pre = (y - inp['rm'].to(dtype)) / torch.sqrt(inp['rv'].to(dtype) + EPS) * L('g') + L('b')
        if 'skip' in inp:
            pre = pre + L('skip')
        pres.append(('', pre.detach()))
        out = lrelu(pre, inp['slope'])
    elif 'g' in inp:
        out = lrelu(bn(y, '', L('skip') if kind == 'join' else None), inp['slope'])
        if 'keep' in inp:
            out = out * inp['keep'].to(dtype) * (1.0 / (1.0 - inp['p']))
        if 'W2' in inp:
            out = rows_matmul(out, L('W2').t()) + L('b2')
    elif inp.get('stats'):
        res['mean'] = y.detach().mean(0)
        res['rstd'] = 1.0 / torch.sqrt(y.detach().var(0, unbiased=False) + EPS)
    res['out'] = out
    return res, leaves, pres


def block_reference(inp, dtype):
    """Every tensor the case compares, in `dtype`, and '_pre_min' = the smallest |pre-activation| of its LeakyReLUs."""
    res, leaves, pres = _forward(inp, dtype, inp['kind'] != 'eval')
    if inp['kind'] != 'eval':
        loss = (res['out'] * inp['gout'].to(dtype)).sum()
        if 'galias' in inp:                                    # the other consumer of the forked tensor
            loss = loss + ((res['j_out'] if inp['kind'] == 'chain' else leaves['x']) * inp['galias'].to(dtype)).sum()
        loss.backward()
        for k, v in leaves.items():
            if k == 'x' and not inp.get('want_dx', True):
                continue
            res[GRAD_NAMES[k]] = v.grad
    res = {k: v.detach() for k, v in res.items()}
    res['_pre_min'] = min([float(p.abs().min()) for _, p in pres] + [float('inf')])
    return res


def nudge(inp):
    """beta (the join's first, then the block's) moved so that no float64 pre-activation is within TAU of 0: per channel that comes within
    TAU, subtract the z nearest 0 among the midpoints of the gaps of at least 2.2 TAU between neighbouring pre-activations and the points
    1.1 TAU outside their range (test_gpu_pointconv.nudge_beta1's rule).  Returns the number of channels moved."""
    moved = 0
    for pfx in (('j_', '') if inp['kind'] == 'chain' else ('',)):
        if pfx + 'b' not in inp:
            continue
        pre = dict(_forward(inp, torch.float64, False)[2])[pfx]
        b = inp[pfx + 'b'].double().clone()
        for ch in (pre.abs().min(0).values < 1.05 * TAU).nonzero().reshape(-1).tolist():
            p = pre[:, ch].sort().values
            ok = (p[1:] - p[:-1]) >= 2.2 * TAU
            cand = torch.cat([((p[1:] + p[:-1]) / 2)[ok], p[:1] - 1.1 * TAU, p[-1:] + 1.1 * TAU])
            b[ch] -= float(cand[cand.abs().argmin()])
            moved += 1
        inp[pfx + 'b'] = b.float()
    return moved


# ------------------------------------------------------------------ inputs
def nrm(rng, *s):
    return torch.from_numpy(rng.standard_normal(s).astype(np.float32))


def uni(rng, shape, lo, hi):
    return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32))


def bn_inputs(rng, co, pfx=''):
    return {pfx + 'g': uni(rng, (co,), 0.5, 1.5), pfx + 'b': uni(rng, (co,), -0.5, 0.5), pfx + 'rm': uni(rng, (co,), -0.2, 0.2),
            pfx + 'rv': uni(rng, (co,), 0.5, 1.5)}


def make_inputs(kind, rng, m, ci, co, slope=0.1, bias=False, split=None, p=None, c2=None, galias=False, want_dx=True, cj=16, j_slope=0.1,
                skip=None, stats=False, fork=False):
    """x = 0.5 + N(0, 1), W = N(0, 1) / sqrt(Ci), gamma in 0.5 .. 1.5, beta in -0.5 .. 0.5, running mean in -0.2 .. 0.2 and variance in
    0.5 .. 1.5, skip = 0.2 + 0.5 N(0, 1), gout = 0.3 + 0.5 N(0, 1), the alias gradient 0.2 + 0.3 N(0, 1): means away from 0, so that the
    column sums do not cancel.  chain: x [m, cj] -> join -> [m, ci] -> block -> [m, co]."""
    cin = cj if kind == 'chain' else ci
    inp = dict(kind=kind, slope=slope, x=0.5 + nrm(rng, m, cin), W=nrm(rng, co, ci) / np.float32(np.sqrt(ci)), want_dx=want_dx, fork=fork)
    if split is not None:
        inp['x'], inp['xb'] = inp['x'][:, :split].contiguous(), inp['x'][:, split:].contiguous()
    if bias:
        inp['bias'] = uni(rng, (co,), -0.5, 0.5)
    if kind != 'linear':
        inp.update(bn_inputs(rng, co))
    if kind == 'chain':
        inp.update(bn_inputs(rng, ci, 'j_'))
        inp.update(j_W=nrm(rng, ci, cj) / np.float32(np.sqrt(cj)), j_slope=j_slope, skip=0.2 + 0.5 * nrm(rng, m, ci))
    if kind == 'join' or skip:
        inp['skip'] = 0.2 + 0.5 * nrm(rng, m, co)
    if p is not None:
        from crfconv_amd import ops
        inp['p'], inp['seed'] = p, ops.dropout_seed(ci, co)
        inp['keep'] = torch.from_numpy(ops.dropout_keep_mask(inp['seed'], 1, m * co, p).reshape(m, co))      # the first forward of a fresh BatchNorm
    if c2 is not None:
        inp.update(W2=nrm(rng, c2, co) / np.float32(np.sqrt(co)), b2=uni(rng, (c2,), -0.5, 0.5))
    if kind != 'eval':
        inp['gout'] = 0.3 + 0.5 * nrm(rng, m, c2 if c2 is not None else co)
    if galias:
        inp['galias'] = 0.2 + 0.3 * nrm(rng, m, ci)
    if stats:
        inp['stats'] = True
    return inp


def prepare(inp):
    """Nudge, both references, the kink and no-cancellation assertions.  Returns (r32, r64)."""
    moved = nudge(inp)
    r64, r32 = block_reference(inp, torch.float64), block_reference(inp, torch.float32)
    if r64['_pre_min'] != float('inf'):
        print('[kink] %s: %d channels moved, min |pre| %.3e (float32 %.3e)' % (inp['kind'], moved, r64['_pre_min'], r32['_pre_min']), flush=True)
    assert r64['_pre_min'] >= TAU and r32['_pre_min'] >= 0.9 * TAU
    for group in KINDS + (None,):
        size = {k: float(v.abs().max()) for k, v in r64.items() if not k.startswith('_')
                and (k in group if group else not any(k in g for g in KINDS))}
        for k, s in size.items():
            assert s > 1e-3 * max(size.values()), '%s: max|ref64| %.3e against %.3e in its case: change the inputs' % (k, s, max(size.values()))
    return r32, r64


# ------------------------------------------------------------------ the device
ENTRIES = {                                                            # kind -> (entries that must run, entries that must not)
    'linear': (['crfconv_linear_forward', 'crfconv_linear_wgrad'], ['crfconv_gemm']),
    'block': (['crfconv_linear_forward', 'crfconv_bn_apply_from_records', 'crfconv_mlp_backward_add'],
              ['crfconv_gemm_stats', 'crfconv_mlp_small_forward', 'crfconv_mlp_backward', 'crfconv_mlp_backward_add_mask']),
    'join': (['crfconv_linear_forward', 'crfconv_bn_apply_from_records', 'crfconv_add_lrelu_backward', 'crfconv_mlp_backward'],
             ['crfconv_mlp_small_forward_join', 'crfconv_mlp_backward_add']),
    'cat': (['crfconv_linear_forward_cat', 'crfconv_bn_apply_from_records', 'crfconv_mlp_backward_cat'], ['crfconv_cat2', 'crfconv_linear_forward']),
    'dropout': (['crfconv_linear_forward', 'crfconv_bn_coef_from_records', 'crfconv_bn_apply_dropout', 'crfconv_dropout_backward',
                 'crfconv_mlp_backward'], ['crfconv_bn_apply_from_records', 'crfconv_linear_forward_dropout']),
    'dropout_linear': (['crfconv_linear_forward', 'crfconv_bn_coef_from_records', 'crfconv_bn_apply_dropout', 'crfconv_linear_forward_dropout',
                        'crfconv_linear_wgrad', 'crfconv_mlp_backward'], ['crfconv_dropout_backward', 'crfconv_head_forward', 'crfconv_gemm']),
    'chain': (['crfconv_linear_forward', 'crfconv_bn_apply_from_records', 'crfconv_mlp_backward_add_mask', 'crfconv_mlp_backward'],
              ['crfconv_add_lrelu_backward', 'crfconv_mlp_backward_add']),
    'eval': (['crfconv_linear_bn_act'], ['crfconv_gemm_bn_act', 'crfconv_cat2', 'crfconv_linear_forward']),
}
NODES = {'linear': '_LinearBackward', 'block': '_MLPBlockBackward', 'join': '_MLPBlockJoinBackward', 'cat': '_MLPBlockCatBackward',
         'dropout': '_MLPBlockDropoutBackward', 'dropout_linear': '_MLPDropoutLinearBackward'}


def graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [f for f, _ in fn.next_functions]
    return {type(fn).__name__ for fn in seen}


def device_bn(inp, pfx, train=True):
    co = inp[pfx + 'g'].numel()
    bn = torch.nn.BatchNorm1d(co, eps=EPS, momentum=MOM).to(DEV).train(train)
    with torch.no_grad():
        bn.weight.copy_(inp[pfx + 'g']); bn.bias.copy_(inp[pfx + 'b']); bn.running_mean.copy_(inp[pfx + 'rm']); bn.running_var.copy_(inp[pfx + 'rv'])
    return bn


def run(inp):
    """The case on the device: (results, entries called)."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    kind = inp['kind']
    m, co = inp['x'].shape[0], inp['W'].shape[0]
    ci = inp['W'].shape[1]
    P = lambda k: torch.nn.Parameter(dev(inp[k]))
    want_dx = inp.get('want_dx', True)
    T = dict(x=dev(inp['x']).requires_grad_(want_dx and kind != 'eval'), W=P('W'))
    for k in ('xb', 'skip'):
        if k in inp:
            T[k] = dev(inp[k]).requires_grad_(kind != 'eval')
    for k in ('bias', 'W2', 'b2', 'j_W'):
        if k in inp:
            T[k] = P(k)
    bn = device_bn(inp, '', kind != 'eval') if 'g' in inp else None
    bnj = device_bn(inp, 'j_') if kind == 'chain' else None
    names, got = [], {}
    nrec = lf_blocks(m)
    with recorded(names):
        poison((m, co), (m, co), (m, co), (m, ci), (nrec, 4, co), (4 * co,))
        if kind == 'eval':
            before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
            coef = ops.bn_eval_coefs([bn])[1][0]
            got['out'] = ops.linear_bn_act(T['x'], T['W'], coef, inp['slope'], T.get('skip'), T.get('xb'), T.get('bias')).cpu()
            assert got['out'].grad_fn is None
            assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and torch.equal(bn.num_batches_tracked, before[2])
            assert all(n in names for n in ENTRIES[kind][0]) and not any(n in names for n in ENTRIES[kind][1]), names
            return got, names
        alias = None
        if kind == 'linear':
            out, rec = ops.linear(T['x'], T['W'], T.get('bias'), want_stats=True)
            assert rec is not None and tuple(rec.shape) == (nrec, 4, co)
            if inp.get('stats'):
                coef = torch.empty(4 * co, dtype=torch.float32, device=DEV)
                one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
                _lib.call('crfconv_bn_coef_from_records', ptr(rec), m, co, ptr(one), ptr(zero), None, None, MOM, EPS, ptr(coef), stream_ptr())
                got['mean'], got['rstd'] = coef[2 * co:3 * co].cpu(), coef[3 * co:].cpu()
        elif kind == 'block':
            out = ops.mlp_block(T['x'], T['W'], bn, inp['slope'], fork=inp.get('fork', False))
            if inp.get('fork', False):
                out, alias = out
                assert (alias is T['x']) == (not want_dx)
        elif kind == 'join':
            out = ops.mlp_block_join(T['x'], T['W'], bn, T['skip'], inp['slope'])
        elif kind == 'cat':
            out = ops.mlp_block_cat(T['x'], T['xb'], T['W'], bn, True, inp['slope'])
        elif kind == 'dropout':
            out = ops.mlp_block_dropout(T['x'], T['W'], bn, inp['slope'], inp['p'])
        elif kind == 'dropout_linear':
            out = ops.mlp_dropout_linear(T['x'], T['W'], bn, inp['slope'], inp['p'], T['W2'], T['b2'], recompute=False)
        else:
            mask = ops.JoinMask()
            hs = ops.mlp_block_join(T['x'], T['j_W'], bnj, T['skip'], inp['j_slope'], mask=mask)
            out, alias = ops.mlp_block(hs, T['W'], bn, inp['slope'], fork=True, input_mask=mask)
            assert mask.folded and mask.slope == inp['j_slope']
            got['j_out'] = hs.detach().cpu()
        assert out is not None, 'the fused node refused the shape'
        nodes = graph_nodes(out)
        for want in ([NODES['join'], NODES['block']] if kind == 'chain' else [NODES[kind]]):
            assert want in nodes, (want, nodes)
        assert not any(n.startswith('_MLPSmall') for n in nodes), nodes
        got['out'] = out.detach().cpu()
        poison((m, ci), (m, co), (co, ci), (co,), (co,), (m, ci))
        if 'galias' in inp:
            torch.autograd.backward([out, alias], [dev(inp['gout']), dev(inp['galias'])])
        else:
            out.backward(dev(inp['gout']))
        torch.cuda.synchronize()
    for k, v in T.items():
        if k == 'x' and not want_dx:
            assert v.grad is None
            continue
        assert v.grad is not None and tuple(v.grad.shape) == tuple(v.shape), k
        got[GRAD_NAMES[k]] = v.grad.cpu()
    for pfx, b in (('', bn), ('j_', bnj)):
        if b is not None:
            got[pfx + 'dgamma'], got[pfx + 'dbeta'] = b.weight.grad.cpu(), b.bias.grad.cpu()
            got[pfx + 'rm'], got[pfx + 'rv'] = b.running_mean.cpu(), b.running_var.cpu()
            assert int(b.num_batches_tracked) == 1
    yes, no = ENTRIES[kind]
    assert all(n in names for n in yes) and not any(n in names for n in no), ([n for n in yes if n not in names], [n for n in no if n in names])
    return got, names


def judge(site, got, r32, r64):
    """Every tensor of `got` against float64 on its own scale within the site's bound; the rule refuses each zeroed and mis-scaled by 10 x
    its bound."""
    want = set(k for k in r64 if not k.startswith('_'))
    assert set(got) == want, sorted(set(got) ^ want)
    for k in sorted(got):
        g = got[k].detach().cpu()
        b = bound(site, k)
        own_scale(g, r32[k], r64[k], b, site + '.' + k)
        assert rejected(torch.zeros_like(g), r32[k], r64[k], b), '%s.%s zeroed passes' % (site, k)
        assert rejected(g.double() * (1.0 + 10.0 * b), r32[k], r64[k], b), '%s.%s mis-scaled by 10 x the bound passes' % (site, k)


def check(site, inp):
    r32, r64 = prepare(inp)
    got, names = run(inp)
    judge(site, got, r32, r64)
    return got, names


@pytest.fixture(autouse=True)
def streaming(monkeypatch):
    """Every row count on the row-streaming family: _mlp_small_ok and the tiled products are out of reach."""
    from crfconv_amd import ops
    monkeypatch.setattr(ops.state, 'mfma_min_rows', 1)
    yield


# ------------------------------------------------------------------ the cases, as data
def case(site, kind, m, ci, co, *what, sub=None, **kw):
    """key: the case's row of BOUNDS -- its site, or site/sub where a few cases of a site are conditioned unlike the others; what: a
    word on what the case is for, beside its make_inputs arguments kw."""
    return dict(site=site, key=site + ('/' + sub if sub else ''), kind=kind, m=m, ci=ci, co=co, what=what, kw=kw)


def build(c):
    rng = seed(*[zlib.crc32((c['site'] + c['kind']).encode()), c['m'], c['ci'], c['co']] + [int(1000 * v) if isinstance(v, float) else int(v or 0)
                                                                                            for v in c['kw'].values()])
    return make_inputs(c['kind'], rng, c['m'], c['ci'], c['co'], **c['kw'])


def forms_of(c):
    """The linear_fwd_kernel instantiations and mlp_plan classes a case launches."""
    kind, ci, co, kw = c['kind'], c['ci'], c['co'], c['kw']
    p1 = tile_plan(c['m'], co, ci, 512, 0)
    cls = {(p1['tco'], p1['tci'])}
    if kind == 'linear':
        return {form(ci, co, False, EPI_NONE), form(co, ci, False, EPI_NONE)}, set()
    if kind == 'eval':
        return {form(ci, co, False, EPI_BN_ACT)}, set()
    fs = {form(ci, co, False, EPI_NONE)}
    if kind == 'chain':
        cj = kw.get('cj', 16)
        pj = tile_plan(c['m'], ci, cj, 512, 0)
        cls.add((pj['tco'], pj['tci']))
        fs |= {form(cj, ci, False, EPI_NONE), form(ci, cj, True, EPI_NONE), form(co, ci, True, EPI_ADD_MASK if kw.get('galias') else EPI_NONE)}
    elif kw.get('want_dx', True):
        fs.add(form(co, ci, True, EPI_ADD if kw.get('galias') else EPI_NONE))
    if kind == 'dropout_linear':
        fs |= {form(co, kw['c2'], False, EPI_NONE), form(kw['c2'], co, False, EPI_DROPOUT)}
    return fs, cls


KS, NS = (12, 24, 48, 96, 144), (8, 20, 52)                    # kernel inputs by NCH class 1, 2, 4, 8, 0; outputs by TCO class 1, 2, 4

LINEAR_FORMS = [(4, 4), (8, 32), (16, 64), (12, 20), (24, 52), (32, 128), (48, 16), (64, 64), (96, 36), (128, 128), (128, 100), (144, 64),
                (256, 64), (512, 32), (6, 32), (32, 13), (7, 5), (24, 36), (100, 12), (50, 52)]
LINEAR_ROWS = [(8, 32), (24, 20), (48, 64), (6, 20)]
LINEAR_MS = (1, 15, 16, 17, 63, 64, 65, 32768 + 19, 2 * 32768 + 5)
BLOCK_WIDTHS = ([(n, k) for k in KS for n in NS] + [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (32, 128), (128, 128), (64, 256), (256, 64),
                                                     (6, 16), (22, 32), (50, 64), (8, 16), (32, 64)])
BOTH_SLOPES = ((8, 16), (32, 64))
BLOCK_ROWS = [(8, 16), (32, 64), (20, 48)]
BLOCK_MS = (2, 17, 63, 64, 65, 129, 2049, 4100, 9300)
REGIME_WIDTHS = [(16, 32), (32, 64)]
FORK_UNALIGNED = [(6, 32), (22, 32), (50, 32)]
JOIN_WIDTHS = [(16, 8), (32, 64), (8, 20)]
CAT_SPLITS = [(4, 28, 32), (12, 20, 32), (16, 16, 32), (64, 64, 64), (24, 8, 16)]
DROPOUT_WIDTHS = [(32, 128, 13), (16, 32, 13), (8, 16, 5), (16, 64, 8), (8, 32, 4), (4, 16, 12)]
EVAL_WIDTHS = [(k, n) for k in KS for n in NS] + [(6, 8), (6, 20), (6, 52)]
SPLITS = {12: 4, 24: 8, 48: 16, 96: 64, 144: 16}


def all_cases():
    cs = []
    for i, (ci, co) in enumerate(LINEAR_FORMS):
        cs.append(case('linear_forms', 'linear', 257, ci, co, bias=i % 2 == 0))
    for ci, co in LINEAR_ROWS:
        for m in LINEAR_MS:
            cs.append(case('linear_rows', 'linear', m, ci, co, bias=m % 2 == 0, stats=True))
    for i, (ci, co) in enumerate(BLOCK_WIDTHS):
        for s in ((0.1, 1.0) if (ci, co) in BOTH_SLOPES else ((0.1, 1.0)[i % 2],)):
            cs.append(case('block_widths', 'block', 333, ci, co, slope=s))
    for ci, co in BLOCK_ROWS:
        for m in BLOCK_MS:
            cs.append(case('block_rows', 'block', m, ci, co, sub='2' if m == 2 else None))
    for k in KS:
        for n in NS:
            cs.append(case('fork_and_mask', 'block', 150, n, k, fork=True, galias=True))
            cs.append(case('fork_and_mask', 'chain', 150, n, k, galias=True, j_slope=(0.3, 0.01)[(k + n) % 8 == 0]))
    for ci, co in FORK_UNALIGNED:
        cs.append(case('fork_and_mask', 'block', 150, ci, co, fork=True, galias=True))
    for ci, co in ((8, 24), (52, 48), (6, 32)):
        cs.append(case('fork_and_mask', 'block', 150, ci, co, 'no alias gradient', fork=True))
        cs.append(case('fork_and_mask', 'block', 150, ci, co, 'no dX', fork=True, want_dx=False))
    for ci, co in ((8, 24), (52, 48)):
        cs.append(case('fork_and_mask', 'chain', 150, ci, co, 'no second consumer', j_slope=0.3))
    for ci, co in JOIN_WIDTHS:
        for s in (0.01, 0.1):
            cs.append(case('join', 'join', 301, ci, co, slope=s))
    for a, b, co in CAT_SPLITS:
        cs.append(case('cat', 'cat', 301, a + b, co, split=a))
    for i, (ci, co, c2) in enumerate(DROPOUT_WIDTHS):
        for p in (0.5, 0.1):
            cs.append(case('dropout', 'dropout_linear', 301, ci, co, p=p, c2=c2))
            if i < 2:
                cs.append(case('dropout', 'dropout', 301, ci, co, p=p))
    for i, (ci, co) in enumerate(EVAL_WIDTHS):
        cs.append(case('eval', 'eval', 257, ci, co, slope=(1.0, 0.1)[i & 1], skip=bool(i & 2), bias=bool(i & 4),
                       split=SPLITS[ci] if (i & 8 or i == 7) and ci in SPLITS else None))
    return cs


def regime_inputs(regime, ci, co):
    """The three regimes of test_block_regimes at M = 333."""
    rng = seed(5, ci, co, len(regime))
    inp = make_inputs('block', rng, 333, ci, co)
    if regime == 'shifted':                                    # x with mean 100 and sigma 1: the shifted sums of the records
        inp['x'] = 100.0 + nrm(rng, 333, ci)
    elif regime == 'small gradient':                           # a mean loss over 10^5 points; column means near 0
        g = rng.standard_normal((333, co))
        inp['gout'] = torch.from_numpy((1e-5 * (g - g.mean(0))).astype(np.float32))
    else:                                                      # column 3 of y = 2 + 1e-3 x (a combination of the other inputs)
        inp['x'][:, 0] = 1.0
        inp['W'][3] = 1e-3 * inp['W'][3]
        inp['W'][3, 0] = 2.0
    return inp


REGIMES = ('shifted', 'small gradient', 'constant column')


def cases_of(site, **match):
    return [c for c in all_cases() if c['site'] == site and all(c[k] == v for k, v in match.items())]


@contextlib.contextmanager
def torch_seed(value=2028):
    """ops.dropout_seed is a function of torch.initial_seed(), which differs from process to process: the CPU generator seeded with
    `value` inside the block (the mask of a case is then the same in every run), its state put back afterwards."""
    state = torch.get_rng_state()
    torch.default_generator.manual_seed(value)
    try:
        yield
    finally:
        torch.set_rng_state(state)


def run_cases(cs):
    assert cs
    out = []
    for c in cs:
        with torch_seed():
            inp = build(c)
            out.append((c, inp) + check(c['key'], inp))
    return out


# ------------------------------------------------------------------ 0: the union of the cases
def test_every_form_is_reached():
    """The cases of this file reach EVERY (TCO, VEC4, NCH, EPI, PRO) for which lf_form is true, except the EPI_UV operand fold, and every
    (tco, tci) class of mlp_plan's switch; every width of theirs fits LDS.  No launch."""
    forms, classes = set(), set()
    for c in all_cases():
        f, p = forms_of(c)
        forms |= f
        classes |= p
    for regime in REGIMES:
        for ci, co in REGIME_WIDTHS:
            f, p = forms_of(case('block_regimes', 'block', 333, ci, co))
            forms |= f
            classes |= p
    assert forms == every_form(), (sorted(every_form() - forms), sorted(forms - every_form()))
    assert classes == set(constants()['P1']), sorted(set(constants()['P1']) ^ classes)
    assert len(every_form()) == 93


# ------------------------------------------------------------------ 1: ops.linear, every reachable (TCO, VEC4, NCH)
@pytest.mark.parametrize('ci,co', LINEAR_FORMS)
def test_linear_forms(ci, co):
    """ops.linear forward, dX (the transposed product) and dW / db at M = 257 (five workgroups, the last with one row), with and without a
    bias.  Ci classes <= 16, 17-32, 33-64, 65-128 (hoisted loops of 1, 2, 4, 8 chunks), above 128 (rolled; 256 and 512: LDS halves TCO), not a
    multiple of 4 (element-wise loads); Ci = 12 a single partial chunk.  Co classes <= 16, 17-48, >= 49 (TCO 1, 2, 4), above 64 (a second
    column slab), not a multiple of 16 (20, 52, 100, 36) or of 4 (13, 5: element-wise stores).  Bounds and CPU e32: BOUNDS['linear_forms']."""
    g, gt = geometry(ci, co, 257, False)['lf'], geometry(co, ci, 257, False)['lf']
    assert g['fits'] and gt['fits'] and g['gx'] == 5
    if ci in (256, 512):
        assert g['tco'] < min(4, max(1, co // 16)) and g['nch'] == 0
    if ci == 12:
        assert g['nch'] == 1 and g['vec4']
    if co > 64 and ci <= 128:
        assert g['gy'] >= 2
    if ci % 4 or co % 4:
        assert not g['vec4'] and g['nch'] == 0
    run_cases(cases_of('linear_forms', ci=ci, co=co))


# ------------------------------------------------------------------ 2: ops.linear and the statistic records over the row counts
@pytest.mark.parametrize('ci,co', LINEAR_ROWS)
def test_linear_rows(ci, co):
    """One width pair per prefetching NCH class (1, 2, 4) and one on the rolled loop, at M = 1, 15, 16, 17 (a partial 16-row group, one
    wavefront), 63, 64, 65 (one workgroup and the first row of a second), cap x 64 + 19 = 32 787 (wavefront 0 of workgroup 0 takes a full
    second row group, wavefront 1 a partial one of 3 rows, every other wavefront none: the prefetched fragments of a group past the end
    are zeros) and 2 x 32 768 + 5.  The statistic records are judged through crfconv_bn_coef_from_records' mean and rstd (gamma = 1,
    beta = 0) against float64; M = 1: one record of one row, variance 0.  Bounds and CPU e32: BOUNDS['linear_rows']."""
    k = constants()
    full = k['CAP'] * (k['LF_BLOCK'] // 64) * 16
    assert full + 19 in LINEAR_MS and 2 * full + 5 in LINEAR_MS
    g = geometry(ci, co, full + 19, False)['lf']
    assert g['pf'] == (ci % 4 == 0) and g['gx'] == k['CAP'] and g['groups'] == (2, 1)
    assert geometry(ci, co, 2 * full + 5, False)['lf']['groups'] == (3, 2) and geometry(ci, co, 17, False)['lf']['gx'] == 1
    run_cases(cases_of('linear_rows', ci=ci, co=co))


# ------------------------------------------------------------------ 3: ops.mlp_block over the widths
@pytest.mark.parametrize('ci,co', BLOCK_WIDTHS)
def test_block_widths(ci, co):
    """ops.mlp_block forward, backward and running statistics at M = 333 (six first-pass slices of 64 rows, the last of 13).  The
    widths reach all eight mlp_bwd_p1_kernel classes, gy > 1 (Co = 48, 96, 144, 256) and gz > 1 (Ci = 52 at Co >= 96, Ci = 256), the
    ticket (Co a power of two up to 128) and the finalize's channel workgroups (Co = 12, 24, 48, 96, 144, 256), unaligned Ci = 6, 22, 50
    (PRO with element-wise stores at TCO 1, 2, 4), every hoisted / rolled PRO form without an epilogue, slopes 0.1 and 1.0 in turn.
    Bounds and CPU e32: BOUNDS['block_widths']."""
    g = geometry(ci, co, 333, True)
    assert g['lf']['fits'] and g['p1']['nblk'] == 6 and g['p1']['rows'] == 64
    assert (g['ticket'] != 'none') == (co in (4, 8, 16, 32, 64, 128))
    assert (g['p1']['gy'] > 1) == (co > 64 or co == 48) and (g['p1']['gz'] > 1) == (ci > 64 or (ci > 32 and co > 48))
    assert g['lf']['vec4'] == (ci % 4 == 0)
    run_cases(cases_of('block_widths', ci=ci, co=co))


# ------------------------------------------------------------------ 4: ops.mlp_block over the row counts
@pytest.mark.parametrize('ci,co', BLOCK_ROWS)
def test_block_rows(ci, co):
    """M = 2, 17, 63, 64, 65, 129 (rows_per_block = 64 > M; one and two slices, one row in the last), 2049, 4100, 9300.  At C = 16 and
    9300 rows bn_apply_plan rounds its 10 row tiles up to 16: six tiles lie past the end.  The first pass draws its ticket flat up to
    LASTWG_FLAT_ = 64 workgroups (M <= 2049 here: 33 slices) and in two levels above (4100: 65 slices, 9300: 146).  M = 1 is left out: the unbiased variance
    divides by n - 1.  At M = 2 the normalised y is +-1 in every channel and the BatchNorm's input gradient cancels down to eps / (var + eps) of
    its terms: dx and dW are what is left of that cancellation (the float32 restatement keeps 1e-4 of them), so these three cases have
    bounds of their own, BOUNDS['block_rows/2'], and do not widen those of the other row counts.  Bounds and CPU e32: BOUNDS['block_rows']."""
    tickets = {m: geometry(ci, co, m, True)['ticket'] for m in BLOCK_MS}
    if co == 16:
        bn = geometry(ci, co, 9300, True)['bn']
        assert bn['live'] == 10 and bn['tiles'] == 16 and bn['rows'] == 1024
    if co in (16, 64):
        assert tickets[2049] == 'flat' and tickets[4100] == tickets[9300] == 'two-level'
        assert geometry(ci, co, 4100, True)['p1_grid'] == constants()['LW_FLAT'] + 1
    else:
        assert set(tickets.values()) == {'none'}
    assert geometry(ci, co, 2, True)['p1']['rows'] == 64 and geometry(ci, co, 129, True)['p1']['nblk'] == 3
    run_cases(cases_of('block_rows', ci=ci, co=co))


# ------------------------------------------------------------------ 5: input regimes
@pytest.mark.parametrize('regime', REGIMES)
def test_block_regimes(regime):
    """ops.mlp_block at M = 333 on x with mean 100 and sigma 1 (the records' shifted sums: y has a column mean of up to ~100 sigma), on an
    upstream gradient of size 1e-5 with column means near 0, and with a column of y that is constant up to 1e-3 (rstd ~ 10^3 amplifies its
    roundings: every regime has bounds of its own).  Bounds and CPU e32: BOUNDS['block_regimes/<regime>']."""
    for ci, co in REGIME_WIDTHS:
        inp = regime_inputs(regime, ci, co)
        if regime == 'small gradient':
            assert float(inp['gout'].mean(0).abs().max()) < 1e-11 and 1e-5 < float(inp['gout'].abs().max()) < 1e-4
        if regime == 'constant column':
            y = inp['x'].double() @ inp['W'].double().t()
            assert float(y[:, 3].std()) < 2e-3 and abs(float(y[:, 3].mean()) - 2.0) < 1e-2
        check('block_regimes/' + regime, inp)


# ------------------------------------------------------------------ 6: the fork, the addend and the masked dX epilogue
@pytest.mark.parametrize('k', KS)
def test_fork_and_mask(k):
    """mlp_block(fork=True) at Co = k and Ci = 8, 20, 52 (M = 150): with a gradient through the alias (crfconv_mlp_backward_add with dX_add:
    EPI_ADD at every TCO and NCH), and the chain mlp_block_join(mask) -> mlp_block(fork=True, input_mask) whose alias has a second
    consumer (crfconv_mlp_backward_add_mask with dX_add: EPI_ADD_MASK; the mask reference is the join's output, the join's slope 0.3 or
    0.01 beside the block's 0.1, so that neither can stand in for the other).  The join's backward then takes the block's dX as its g1: its
    dskip, dx, dW are judged too.  At k = 24 and 48 also: the alias without a gradient, requires_grad off for x (no dX), and the chain
    without a second consumer (the plain product, then the mask pass in place); at k = 12 the unaligned Ci = 6, 22, 50 (EPI_ADD with element-wise stores).  Bounds and CPU e32: BOUNDS['fork_and_mask']."""
    cs = cases_of('fork_and_mask', co=k) + (cases_of('fork_and_mask', co=32) if k == 12 else [])
    assert len(cs) >= 6
    for c, inp, got, names in run_cases(cs):
        if c['kind'] == 'chain':
            assert names.count('crfconv_mlp_backward_add_mask') == 1 and names.count('crfconv_mlp_backward') == 1


# ------------------------------------------------------------------ 7: the join
@pytest.mark.parametrize('ci,co', JOIN_WIDTHS)
def test_join(ci, co):
    """mlp_block_join at join slopes 0.01 and 0.1, M = 301: C = 8 (a partial 16-channel slab of bn_apply_records_kernel<true>), 20 (a
    second, partial slab) and 64; the pre-activation nudged away from 0 includes + skip; the gradient to skip is judged.  Bounds and CPU e32:
    BOUNDS['join']."""
    assert geometry(ci, co, 301, False)['bn']['slabs'] == cdiv(co, 16)
    for c, inp, got, names in run_cases(cases_of('join', ci=ci, co=co)):
        assert 'dskip' in got


# ------------------------------------------------------------------ 8: the two-pointer operand
@pytest.mark.parametrize('a,b,co', CAT_SPLITS)
def test_cat(a, b, co):
    """mlp_block_cat at the splits 4 | 28, 12 | 20 (inside a 16-chunk), 16 | 16 (on a chunk boundary), 64 | 64 and 24 | 8, M = 301: the
    forward reads [xa | xb] through two pointers, the backward writes both input gradients, and both are judged.  Bounds and CPU e32:
    BOUNDS['cat']."""
    for c, inp, got, names in run_cases([c for c in cases_of('cat', ci=a + b, co=co) if c['kw']['split'] == a]):
        assert tuple(got['dx'].shape) == (301, a) and tuple(got['dxb'].shape) == (301, b)


# ------------------------------------------------------------------ 9: dropout
@pytest.mark.parametrize('ci,co,c2', DROPOUT_WIDTHS)
def test_dropout(ci, co, c2):
    """mlp_dropout_linear(recompute=False) at p = 0.5 and 0.1, M = 301, and mlp_block_dropout at the first two width triples: the mask is
    ops.dropout_keep_mask with the node's seed and the BatchNorm's counter after the forward (1), the share of kept elements within 5
    standard deviations of 1 - p.  The masked input gradient of the last Linear is crfconv_linear_forward_dropout with c2 inputs: c2 = 13
    and 5 take the unaligned forms at TCO 4, 2, 1, c2 = 8, 4, 12 the aligned ones.  The dropped elements of mlp_block_dropout's output
    are exact zeros.  Bounds and CPU e32: BOUNDS['dropout']."""
    for c, inp, got, names in run_cases(cases_of('dropout', ci=ci, co=co)):
        n, p = inp['keep'].numel(), inp['p']
        assert abs(float(inp['keep'].double().mean()) - (1.0 - p)) <= 5.0 * np.sqrt(p * (1.0 - p) / n)
        if c['kind'] == 'dropout':
            assert bool((got['out'][~inp['keep']] == 0).all()) and bool((got['out'][inp['keep']] != 0).all())


# ------------------------------------------------------------------ 10: the eval-mode block as one launch
@pytest.mark.parametrize('k', KS + (6,))
def test_eval(k):
    """ops.linear_bn_act in its streaming range at Ci = k and Co = 8, 20, 52 (M = 257): EPI_BN_ACT at every TCO and NCH and, Ci = 6,
    unaligned; with and without skip, the second operand xb, a bias, at slopes 1 and 0.1 -- the sixteen combinations are spread over the
    cases.  The BatchNorm's running tensors and num_batches_tracked are bit-identical before and after (`run`).  Bounds and CPU e32:
    BOUNDS['eval']."""
    run_cases(cases_of('eval', ci=k))


def test_eval_options_are_all_met():
    """The eighteen eval cases meet skip, xb, bias and both slopes in every pairing of two of them.  No launch."""
    flags = [(c['kw']['slope'] != 1.0, c['kw']['skip'], c['kw']['bias'], c['kw']['split'] is not None) for c in cases_of('eval')]
    for i in range(4):
        for j in range(i + 1, 4):
            assert {(f[i], f[j]) for f in flags} == {(a, b) for a in (False, True) for b in (False, True)}, (i, j)


# ------------------------------------------------------------------ the CPU column of BOUNDS
def cpu_profile():
    """The float32 restatement of every case against the float64 one, on the CPU: prints, per (site, tensor), the largest e32 and the bound
    it gives (10 x, rounded up to one digit, at least 1e-6), and checks e32 against BOUNDS where BOUNDS has the pair."""
    import math
    worst, n = {}, 0
    with torch_seed():
        todo = [(c['key'], build(c)) for c in all_cases()]
    todo += [('block_regimes/' + r, regime_inputs(r, ci, co)) for r in REGIMES for ci, co in REGIME_WIDTHS]
    for site, inp in todo:
        r32, r64 = prepare(inp)
        n += 1
        for k in r64:
            if not k.startswith('_'):
                e32 = errors(r32[k], r32[k], r64[k])[1]
                worst.setdefault(site, {})[k] = max(worst.get(site, {}).get(k, 0.0), e32)
    print('%d cases' % n)
    for site, d in worst.items():
        row = []
        for k, e32 in d.items():
            mag = 10.0 ** math.floor(math.log10(10.0 * e32)) if e32 > 0 else 1e-6
            b = max(math.ceil(10.0 * e32 / mag - 1e-9) * mag, 1e-6)
            row.append('%s=(%.0e, %.1e, None)' % (k, b, e32))
            if site in BOUNDS and k in BOUNDS[site]:
                assert e32 <= BOUNDS[site][k][0], (site, k, e32)
        print("    '%s': dict(%s)," % (site, ', '.join(row)))


if __name__ == '__main__':
    cpu_profile()
