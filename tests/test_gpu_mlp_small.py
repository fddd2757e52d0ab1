"""-m gpu: the coarse dense stack -- every Linear -> BatchNorm -> LeakyReLU below ops.state.mfma_min_rows rows -- form by form, against
the float64 reference of test_gpu_mlp_stream (`block_reference`: plain torch with autograd on the CPU, row products in 64-row blocks):
the one-launch forward of csrc/mlp_small.hip in its three tile widths, without and with the ResNet join; the tiled product with
statistic records (csrc/gemm_stats.hip, the STATS form of gemm_tile.hpp, narrow and wide tiles) and the BatchNorm apply from its
16-row-group records (csrc/bn_records.hip); the fused backward of csrc/mlp_small_bwd.hip (tile sums with the last-workgroup ticket, the
PRO product with gY formed on operand load, with the addend and the masked epilogue) as one launch and as two; the fallback backward
(crfconv_bn_backward + crfconv_gemm) behind either forward; the group node (crfconv_gemm_stats_jobs,
crfconv_bn_apply_from_records_jobs, up to four jobs per backward launch).

Nothing is forced: this file does NOT set mfma_min_rows.  Every case has fewer than 12288 rows, so _mlp_small_ok routes it into the family on
its own; each case asserts the autograd node it expects (_MLPSmallBackward, _MLPSmallJoinBackward, _MLPSmallGroupBackward), that no
_MLPBlock* node is in the graph, and which library entries ran and which did not (test_gpu_pointconv's `recorded`).  Everything goes
through ops.mlp_block, ops.mlp_block_join and ops.mlp_group, except one raw call of crfconv_mlp_small_backward with training = 0, a
branch the wrappers never take.

Reference and rule are test_gpu_mlp_stream's, unchanged: `prepare` (nudge + both references + its kink and no-cancellation assertions)
passes for every case, no LeakyReLU branch is taken from the kernel, no channel or element is left out; per tensor
e = max|got - ref64| / max|ref64| <= max(bound, 4 e32) with e32 <= bound asserted (test_gpu_discrete's `own_scale`), each tensor refused
when zeroed and when mis-scaled by 10 x its bound, the allocator poisoned before every forward and backward.  A bound belongs to a
(site, tensor) pair (BOUNDS): 10 x the largest e32 the float32 restatement showed on the CPU over the site's cases, rounded up to one
digit, never below 1e-6.  `python tests/test_gpu_mlp_small.py` runs the restatements of every case without a GPU and prints that
column.  The cases with M = 2 are conditioned unlike the rest (test_gpu_mlp_stream.test_block_rows says why) and have rows of their own,
site/2.

The kernels' geometry is READ from the sources (`constants`): SM_ROWS, SM_COLS, SM_KC, SM_MAX_ROWS_, SM_MIN_BLOCKS, mlp_small_shape_ok,
mlp_small_tco, GM_BK_, GM_WIDE_MIN_N_, GM_WIDE_MIN_TILES_, gm_wide, gm_tile_plan, GM_PRO_MAXK, GG_MAX, BT_ROWS, BT_CH, bt_plan with
BT_MAXTILES and the 24-tile round of the last workgroup's sum, crfconv_gemm_stat_records, BNS_ROWS and BNS_NR, each restated beside a
regular expression over the text it restates.  The co-residency capacity is not exported: `capacity` infers it once per session from
crfconv_mlp_small_supported(4096, 16, 64 k), k = 1 .. 16.  Every case states the form it is for and asserts, through the restatement,
that it takes it; test_every_form_is_reached asserts that the union of the cases reaches every form of FORMS.

Not here, and held today by: the UV operand forms crfconv_mlp_small_forward_join_uv / crfconv_gemm_stats_uv (test_gpu_operand_fold.py),
the eval epilogue crfconv_gemm_bn_act (test_gpu_infer.py), plain crfconv_gemm tile shapes and odd widths (test_gpu_model.py), graph
replay of the barrier kernels (test_gpu_model.py), deferred weight-gradient delivery (test_gpu_mlp_nodes.py,
test_gpu_backward_tail.py), a grid barrier or in-launch wait that gives up (test_grid_barrier_failure_*), head.hip, loss.hip and the
stand-alone statistics pass of bn.hip (test_gpu_model.py, test_gpu_infer.py, test_gpu_native.py).  Measured figures per site: BOUNDS and
profiles/r30_mlp_small_float64.md."""
import functools
import os
import re
import sys

import pytest
import torch

if __name__ == '__main__':                                     # the CPU column of BOUNDS: no pytest, no GPU
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_util import DEV
from test_gpu_discrete import dev, errors, own_scale, poison, rejected
from test_gpu_mlp_stream import (EPS, GRAD_NAMES, KINDS, REGIMES, TAU, block_reference, build, case, cdiv, device_bn, graph_nodes,
                                 make_inputs, nudge, prepare, regime_inputs, torch_seed)
from test_gpu_pointconv import _csrc_int, _src, recorded, rows_matmul, seed

pytestmark = pytest.mark.gpu

# site -> tensor -> (bound, largest e32 of the float32 restatement on the CPU, largest e measured on the MI355X).  bound = 10 x the e32 of
# the CPU run made BEFORE the GPU run, rounded up to one digit, never below 1e-6; the e32 recorded here is the larger of that run's and of
# the restatement on the MI355X machine's host CPU (profiles/r30_mlp_small_float64.md lists both).
BOUNDS = {
    'one_launch_tiles/2': dict(rm=(1e-06, 9.4e-08, 7.1e-08), rv=(1e-06, 8.4e-08, 8.4e-08), out=(2e-04, 1.4e-05, 6.8e-06), dx=(3e-04, 2.4e-05, 3.5e-06),
                               dW=(2e-04, 1.2e-05, 3.7e-06), dgamma=(2e-04, 1.2e-05, 3.5e-06), dbeta=(1e-06, 3.4e-08, 3.4e-08)),
    'one_launch_tiles': dict(rm=(2e-06, 1.2e-07, 7.6e-08), rv=(2e-06, 1.0e-07, 5.3e-08), out=(8e-06, 7.3e-07, 1.5e-06), dx=(7e-06, 6.4e-07, 1.3e-06),
                             dW=(1e-05, 9.7e-07, 7.2e-07), dgamma=(8e-06, 7.0e-07, 4.8e-07), dbeta=(2e-06, 1.4e-07, 5.3e-08)),
    'tiled_forward/2': dict(rm=(1e-06, 8.3e-08, 1.9e-08), rv=(1e-06, 8.9e-08, 4.4e-08), out=(1e-06, 1.2e-07, 8.6e-08), dx=(2e-03, 1.9e-04, 4.8e-05),
                            dW=(2e-03, 1.9e-04, 4.4e-05), dgamma=(1e-06, 6.4e-08, 5.0e-08), dbeta=(1e-06, 2.2e-08, 2.2e-08)),
    'tiled_forward': dict(rm=(2e-06, 1.0e-07, 3.9e-08), rv=(1e-06, 9.8e-08, 4.7e-08), out=(7e-06, 6.0e-07, 6.0e-07), dx=(8e-06, 7.9e-07, 5.6e-07),
                          dW=(2e-05, 1.7e-06, 1.2e-06), dgamma=(3e-06, 3.1e-07, 2.0e-07), dbeta=(2e-06, 1.4e-07, 4.7e-08)),
    'fused_backward/2': dict(rm=(1e-06, 7.5e-08, 8.3e-08), rv=(1e-06, 7.9e-08, 5.4e-08), out=(2e-05, 1.6e-06, 1.3e-06), dx=(2e-03, 1.7e-04, 2.3e-04),
                             dW=(9e-04, 8.9e-05, 1.4e-04), dgamma=(5e-06, 4.9e-07, 5.0e-07), dbeta=(1e-06, 3.8e-08, 3.8e-08)),
    'fused_backward': dict(rm=(2e-06, 1.3e-07, 4.9e-08), rv=(1e-06, 9.8e-08, 5.3e-08), out=(7e-06, 6.8e-07, 5.9e-07), dx=(6e-06, 5.4e-07, 1.1e-06),
                           dW=(2e-05, 2.6e-06, 1.4e-06), dgamma=(4e-06, 3.4e-07, 3.1e-07), dbeta=(2e-06, 1.8e-07, 6.8e-08),
                           j_rm=(1e-06, 7.9e-08, 3.4e-08), j_rv=(1e-06, 8.2e-08, 4.5e-08), j_out=(4e-06, 3.1e-07, 2.5e-07),
                           j_dW=(9e-06, 1.1e-06, 1.1e-06), dskip=(4e-06, 3.8e-07, 3.5e-07), j_dgamma=(4e-06, 3.8e-07, 4.0e-07),
                           j_dbeta=(2e-05, 1.2e-06, 5.9e-07)),
    'fallback_backward': dict(rm=(1e-06, 8.8e-08, 6.1e-08), rv=(1e-06, 9.4e-08, 4.3e-08), out=(3e-06, 2.9e-07, 2.3e-07), dx=(6e-06, 5.1e-07, 1.2e-06),
                              dW=(2e-05, 1.6e-06, 7.0e-07), dgamma=(3e-06, 2.7e-07, 1.4e-07), dbeta=(2e-06, 1.4e-07, 5.7e-08)),
    'join': dict(rm=(2e-06, 1.0e-07, 5.5e-08), rv=(1e-06, 9.2e-08, 4.6e-08), out=(5e-06, 4.0e-07, 3.4e-07), dx=(7e-06, 6.5e-07, 9.1e-07),
                 dW=(2e-05, 1.9e-06, 6.8e-07), dskip=(1e-06, 4.6e-09, 4.6e-09), dgamma=(2e-05, 1.1e-06, 6.9e-07), dbeta=(2e-06, 1.4e-07, 6.1e-08)),
    'group': dict(rm=(2e-06, 1.1e-07, 4.8e-08), rv=(1e-06, 9.0e-08, 5.5e-08), out=(5e-06, 5.6e-07, 4.7e-07), dx=(5e-06, 5.0e-07, 4.8e-07),
                  dW=(2e-05, 1.5e-06, 1.4e-06), dgamma=(3e-05, 2.3e-06, 1.2e-06), dbeta=(2e-06, 1.6e-07, 5.5e-08), j_rm=(1e-06, 7.9e-08, 3.9e-08),
                  j_rv=(1e-06, 9.4e-08, 5.0e-08), j_out=(3e-06, 2.0e-07, 1.5e-07), j_dW=(4e-06, 3.6e-07, 3.2e-07), dskip=(2e-06, 1.9e-07, 1.8e-07),
                  j_dgamma=(3e-06, 2.7e-07, 1.7e-07), j_dbeta=(3e-06, 2.1e-07, 1.8e-07)),
    'eval_backward': dict(gY=(1e-06, 3.7e-08, 3.7e-08), dx=(5e-06, 4.2e-07, 2.3e-07), dbeta=(4e-06, 3.8e-07, 4.6e-08),
                          dgamma=(4e-06, 4.7e-07, 6.7e-08)),
    'regimes/shifted': dict(rm=(3e-06, 2.0e-07, 3.7e-08), rv=(5e-06, 4.8e-07, 2.9e-07), out=(3e-04, 3.0e-05, 2.4e-05), dx=(9e-05, 8.5e-06, 4.1e-06),
                            dW=(9e-02, 8.3e-03, 1.8e-03), dgamma=(8e-04, 7.5e-05, 1.6e-05), dbeta=(2e-06, 1.1e-07, 5.8e-08)),
    'regimes/small gradient': dict(rm=(1e-06, 8.9e-08, 3.7e-08), rv=(1e-06, 8.6e-08, 4.4e-08), out=(3e-06, 2.7e-07, 2.4e-07),
                                   dx=(4e-06, 3.0e-07, 2.9e-07), dW=(2e-06, 1.9e-07, 2.1e-07), dgamma=(3e-06, 2.3e-07, 2.1e-07),
                                   dbeta=(2e-06, 1.3e-07, 8.7e-08)),
    'regimes/constant column': dict(rm=(2e-06, 1.2e-07, 4.4e-08), rv=(1e-06, 7.7e-08, 4.4e-08), out=(8e-04, 7.5e-05, 8.2e-05),
                                    dx=(1e-04, 9.9e-06, 7.3e-06), dW=(4e-04, 3.2e-05, 1.6e-05), dgamma=(2e-03, 1.0e-04, 2.4e-05),
                                    dbeta=(2e-06, 1.2e-07, 5.4e-08)),
}


def bound(key, name):
    return BOUNDS[key][name][0]


# ------------------------------------------------------------------ the kernels' geometry, read from the sources
@functools.lru_cache(maxsize=None)
def constants():
    """The tunables the plans depend on, by name, after checking the text of every formula restated below."""
    sm, gt, gs, bw, bn = _src('mlp_small.hip'), _src('gemm_tile.hpp'), _src('gemm_stats.hip'), _src('mlp_small_bwd.hip'), _src('bn.hip')

    def need(text, *patterns):
        for p in patterns:
            assert re.search(p, text), 'the sources no longer say: %s' % p

    def nums(text, pattern):
        hit = re.search(pattern, text)
        assert hit, 'the sources no longer say: %s' % pattern
        return [int(v) for v in hit.groups()]
    k = {}
    k['SM_ROWS'], k['SM_COLS'], k['SM_KC'] = nums(sm, r'constexpr int SM_BLOCK = 256, SM_ROWS = (\d+), SM_COLS = (\d+), SM_KC = (\d+), SM_LD = SM_KC \+ 4;')
    k.update(SM_MAX_ROWS=_csrc_int('mlp_small.hip', 'SM_MAX_ROWS_'), SM_MIN_BLOCKS=_csrc_int('mlp_small.hip', 'SM_MIN_BLOCKS'),
             GM_BK=_csrc_int('gemm_tile.hpp', 'GM_BK_'), WIDE_MIN_N=_csrc_int('gemm_tile.hpp', 'GM_WIDE_MIN_N_'),
             WIDE_MIN_TILES=_csrc_int('gemm_tile.hpp', 'GM_WIDE_MIN_TILES_'), PRO_MAXK=_csrc_int('gemm_tile.hpp', 'GM_PRO_MAXK'),
             GG_MAX=_csrc_int('gemm_tile.hpp', 'GG_MAX'))
    need(sm, r'constexpr int64_t SM_MAX_ROWS = SM_MAX_ROWS_;', r'const int r = rb \* SM_ROWS \+ wave \* 16 \+ rr;', r'constexpr int COLS = 16 \* TCO;',
         r'for \(int kc = 0; kc < Ci; kc \+= SM_KC\) \{',
         # mlp_small_shape_ok
         r'return M >= 1 && M <= SM_MAX_ROWS && Ci >= 16 && Ci % 16 == 0 && Ci <= 1024 && Co >= SM_COLS && Co % SM_COLS == 0 && Co <= 1024;',
         # mlp_small_tco
         r'const int64_t rb = cdiv\(M, SM_ROWS\);\s*for \(int tco = 4; tco >= 1; tco >>= 1\) \{\s*const int64_t nblk = rb \* \(Co / \(16 \* tco\)\);',
         r'if \(nblk > cap\) return 0;', r'if \(nblk >= SM_MIN_BLOCKS \|\| tco == 1\) return tco;',
         r'return mlp_small_tco\(M, Co, mlp_small_capacity\(\)\) > 0 \? 1 : 0;', r'if \(per_cu > 2\) per_cu = 2;',
         # the record of a wavefront without rows, and who skips it
         r'sw\[COLS \+ cl\] = \(float\)nrows;', r'if \(nb <= 0\.0\) continue;',
         r'constexpr int PARTS = SM_BLOCK / COLS, NB = \(int\)\(SM_MAX_ROWS / SM_ROWS\) / PARTS;')
    # gm_wide, gm_tile_plan, the two tile classes of the job kernels
    need(gt, r'return N >= GM_WIDE_MIN_N_ && \(\(M \+ 31\) / 32\) \* \(int64_t\)\(\(N \+ 31\) / 32\) >= GM_WIDE_MIN_TILES_;',
         r'p\.tiles_x = \(int\)\(\(M \+ 31\) / 32\);', r'p\.wide = may_be_wide && gm_wide\(M, N\) \? 1 : 0;',
         r'p\.tiles = \(int64_t\)p\.tiles_x \* \(\(N \+ \(p\.wide \? 63 : 31\)\) / \(p\.wide \? 64 : 32\)\);',
         r'const int nchunk = \(K \+ GM_BK - 1\) / GM_BK;', r'const int rec = \(int\)bx \* WR \+ wr;')
    need(gs, r'gemm_tile<1, 2, 2, 2, true, true, false, true>', r'gemm_tile<1, 1, 2, 2, true, true, false, true>',
         r'if \(int rc = crf::gm_tile_plan\(b\.M, b\.N, true, tiles, p\)\) return rc;',
         # crfconv_gemm_stat_records
         r'return M < 1 \? 0 : \(size_t\)\(2 \* \(\(M \+ 31\) / 32\)\);')
    # the tile sums: bt_plan, the last workgroup's rounds, the widths the fused backward takes
    k['BT_ROWS'], k['BT_CH'] = nums(bw, r'constexpr int BT_ROWS = (\d+), BT_CH = (\d+), BT_NR = BT_ROWS / 16;')
    k['BT_MAXTILES'], = nums(bw, r'constexpr int BT_MAXTILES = (\d+);')
    k['BT_ROUND'], = nums(bw, r'for \(int t0 = 0; t0 < f\.ntile; t0 \+= (\d+)\) \{\s*double v\[24\];')
    need(bw, r'int64_t rows = crf::BT_ROWS;\s*if \(\(M \+ rows - 1\) / rows > BT_MAXTILES\) rows = \(\(\(M \+ BT_MAXTILES - 1\) / BT_MAXTILES \+ 15\) / 16\) \* 16;',
         r'ntile = \(int\)\(\(M \+ rows - 1\) / rows\);', r'for \(int base = row0; base < row_end; base \+= BT_ROWS\) \{',
         r'return \(M >= 1 && M < \(int64_t\)1 << 24 && Ci >= 4 && Co >= 4 && Ci % 4 == 0 && Co % 4 == 0 && Co <= crf::GM_PRO_MAXK\) \? 1 : 0;',
         r'if \(int rc = crf::gm_tile_plan\(b\.M, b\.Ci, true, tiles \+ blocks, p\)\) return rc;',
         r'blocks \+= \(int64_t\)ntile \* \(\(b\.Co \+ crf::BT_CH - 1\) / crf::BT_CH\);')
    # bn.hip: the register-resident BatchNorm backward of the fallback
    k['BNS_NR'], = nums(bn, r'constexpr int BNS_BLOCK = 1024, BNS_CH = 4, BNS_ROWS = BNS_BLOCK, BNS_NR = (\d+), BNS_MAXM = BNS_ROWS \* BNS_NR;')
    k['BNS_ROWS'] = 1024
    need(bn, r'static bool bn_small_ok\(int64_t M, int C\) \{ return M <= BNS_MAXM && C % BNS_CH == 0; \}',
         r'if \(bn_small_ok\(M, C\)\) \{\s*if \(M <= BNS_ROWS\)\s*hipLaunchKernelGGL\(bn_small_bwd_kernel<1>',
         r'hipLaunchKernelGGL\(bn_small_bwd_kernel<BNS_NR>', r'hipLaunchKernelGGL\(bn_bwd_reduce_kernel')
    return k


def sm_shape_ok(m, ci, co):
    k = constants()
    return 1 <= m <= k['SM_MAX_ROWS'] and ci >= 16 and ci % 16 == 0 and ci <= 1024 and co >= k['SM_COLS'] and co % k['SM_COLS'] == 0 and co <= 1024


def sm_tco(m, co, cap):
    """mlp_small_tco: 16-channel tiles per workgroup of the one-launch forward, 0 = its workgroups cannot all be resident."""
    k = constants()
    rb = cdiv(m, k['SM_ROWS'])
    for tco in (4, 2, 1):
        nblk = rb * (co // (16 * tco))
        if nblk > cap:
            return 0
        if nblk >= k['SM_MIN_BLOCKS'] or tco == 1:
            return tco
    return 0


def gm_wide(m, n):
    k = constants()
    return n >= k['WIDE_MIN_N'] and cdiv(m, 32) * cdiv(n, 32) >= k['WIDE_MIN_TILES']


def gm_tile_plan(m, n):
    """(tiles_x, wide, tiles) of a job of the 32-row forms."""
    wide = gm_wide(m, n)
    return cdiv(m, 32), wide, cdiv(m, 32) * cdiv(n, 64 if wide else 32)


def bt_plan(m):
    """(ntile, tile_rows) of the tile sums."""
    k = constants()
    rows = k['BT_ROWS']
    if cdiv(m, rows) > k['BT_MAXTILES']:
        rows = cdiv(cdiv(m, k['BT_MAXTILES']), 16) * 16
    return cdiv(m, rows), rows


def bwd_fused_ok(m, ci, co):
    return 1 <= m < 1 << 24 and ci >= 4 and co >= 4 and ci % 4 == 0 and co % 4 == 0 and co <= constants()['PRO_MAXK']


def stat_records(m):
    return 2 * cdiv(m, 32)


def layer_forms(m, ci, co, cap, join=False, want_dx=True, group=False):
    """The forms one Linear -> BatchNorm (-> LeakyReLU) of x [m, ci] -> [m, co] takes, forward and backward."""
    k = constants()
    f = set()
    tco = 0 if group or not sm_shape_ok(m, ci, co) else sm_tco(m, co, cap)
    f.add(('fwd', tco, join) if tco else ('tiled', gm_wide(m, co)))
    if group or (want_dx and bwd_fused_ok(m, ci, co)):
        ntile, rows = bt_plan(m)
        f.add(('pro', gm_wide(m, ci)))
        f.add(('sums', '1' if ntile == 1 else ('2..24' if ntile <= k['BT_ROUND'] else '25..48')))
        if rows > k['BT_ROWS']:
            f.add(('sums', 'long'))
    else:
        f.add(('fallback', '1' if m <= k['BNS_ROWS'] else ('3' if m <= k['BNS_ROWS'] * k['BNS_NR'] else 'stream')))
    return f


FORMS = ({('fwd', t, j) for t in (1, 2, 4) for j in (False, True)} | {('tiled', False), ('tiled', True), ('pro', False), ('pro', True)}
         | {('sums', s) for s in ('1', '2..24', '25..48', 'long')} | {('entry', 'one'), ('entry', 'two')}
         | {('fallback', s) for s in ('1', '3', 'stream')} | {('group', n) for n in (2, 3, 4)})
_CAP = []


def capacity():
    """Workgroups of the one-launch forward that can be resident at once, to the granularity of 64: the largest 64 k for which the
    library takes 4096 rows x 64 k channels (64 row blocks x k tiles of 64 channels), inferred once per session."""
    if not _CAP:
        from crfconv_amd import _lib
        lib = _lib.load()
        took = [64 * k for k in range(1, 17) if lib.crfconv_mlp_small_supported(4096, 16, 64 * k) == 1]
        assert took and took == list(range(64, took[-1] + 1, 64)), took
        assert took[-1] > 0 and took[-1] % 64 == 0
        _CAP.append(took[-1])
    return _CAP[0]


# ------------------------------------------------------------------ the device
FAMILY = ('crfconv_mlp_small_forward', 'crfconv_mlp_small_forward_join', 'crfconv_gemm_stats', 'crfconv_bn_apply_from_records',
          'crfconv_mlp_small_backward_jobs_one_launch', 'crfconv_mlp_small_backward_jobs', 'crfconv_bn_backward', 'crfconv_gemm',
          'crfconv_add_lrelu_backward', 'crfconv_gemm_stats_jobs', 'crfconv_bn_apply_from_records_jobs', 'crfconv_add_mask')
NEVER = ('crfconv_linear_forward', 'crfconv_mlp_backward', 'crfconv_mlp_backward_add', 'crfconv_mlp_backward_add_mask',
         'crfconv_mlp_small_forward_join_uv', 'crfconv_gemm_stats_uv', 'crfconv_bn_coef_from_records')
NODES = {'block': '_MLPSmallBackward', 'join': '_MLPSmallJoinBackward'}


def layer_entries(forms, join, one_launch):
    yes = set()
    for f in forms:
        if f[0] == 'fwd':
            yes.add('crfconv_mlp_small_forward_join' if join else 'crfconv_mlp_small_forward')
        elif f[0] == 'tiled':
            yes |= {'crfconv_gemm_stats', 'crfconv_bn_apply_from_records'}
        elif f[0] == 'pro':
            yes.add('crfconv_mlp_small_backward_jobs_one_launch' if one_launch else 'crfconv_mlp_small_backward_jobs')
        elif f[0] == 'fallback':
            yes.add('crfconv_bn_backward')
    return yes


def expected_entries(inp):
    """(entries that must run, entries that must not) of a block / join / chain case in the current backward form."""
    from crfconv_amd import ops
    one = bool(ops.state.small_bwd_one_launch)
    kind, m = inp['kind'], inp['x'].shape[0]
    co, ci = inp['W'].shape
    want_dx = inp.get('want_dx', True)
    yes = layer_entries(layer_forms(m, ci, co, capacity(), kind == 'join', want_dx or kind == 'chain'), kind == 'join', one)
    if kind == 'join':
        yes.add('crfconv_add_lrelu_backward')
    if kind == 'chain':
        yes |= layer_entries(layer_forms(m, inp['j_W'].shape[1], ci, capacity(), True), True, one)
    if want_dx and kind != 'chain' and 'crfconv_bn_backward' in yes:
        yes.add('crfconv_gemm')
    return yes, (set(FAMILY) - yes) | set(NEVER)


def gridsync_is_clean():
    from crfconv_amd import ops
    assert int(ops.gridsync_ws(DEV).abs().sum()) == 0, 'barrier or wait words left non-zero'
    ops.check_gridsync()


def run(inp):
    """A block / join / chain case on the device through the public wrappers: (results, entries called)."""
    from crfconv_amd import ops
    kind = inp['kind']
    m, co = inp['x'].shape[0], inp['W'].shape[0]
    ci = inp['W'].shape[1]
    P = lambda k: torch.nn.Parameter(dev(inp[k]))
    want_dx = inp.get('want_dx', True)
    T = dict(x=dev(inp['x']).requires_grad_(want_dx), W=P('W'))
    if 'skip' in inp:
        T['skip'] = dev(inp['skip']).requires_grad_(True)
    if 'j_W' in inp:
        T['j_W'] = P('j_W')
    bn = device_bn(inp, '')
    bnj = device_bn(inp, 'j_') if kind == 'chain' else None
    names, got = [], {}
    assert not ops.state.small_mlp_disabled and m < ops.state.mfma_min_rows
    with recorded(names):
        poison((m, co), (m, co), (m, co), (m, ci), (stat_records(m), co, 4), (4 * co,))
        alias = None
        if kind == 'block':
            out = ops.mlp_block(T['x'], T['W'], bn, inp['slope'], fork=inp.get('fork', False))
            if inp.get('fork', False):
                out, alias = out
                assert (alias is T['x']) == (not want_dx)
        elif kind == 'join':
            out = ops.mlp_block_join(T['x'], T['W'], bn, T['skip'], inp['slope'])
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
        assert not any(n.startswith('_MLPBlock') for n in nodes), nodes
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
    yes, no = expected_entries(inp)
    assert all(n in names for n in yes) and not any(n in names for n in no), (sorted(yes - set(names)), sorted(no & set(names)))
    return got, names


def judge(key, got, r32, r64, tag=''):
    """Every tensor of `got` against float64 on its own scale within the bound of its (site, tensor); the rule refuses each zeroed and
    mis-scaled by 10 x its bound."""
    want = set(k for k in r64 if not k.startswith('_'))
    assert set(got) == want, sorted(set(got) ^ want)
    for k in sorted(got):
        g = got[k].detach().cpu()
        b = bound(key, k)
        own_scale(g, r32[k], r64[k], b, key + '.' + k + tag)
        assert rejected(torch.zeros_like(g), r32[k], r64[k], b), '%s.%s zeroed passes' % (key, k)
        assert rejected(g.double() * (1.0 + 10.0 * b), r32[k], r64[k], b), '%s.%s mis-scaled by 10 x the bound passes' % (key, k)


# ------------------------------------------------------------------ the cases, as data
K_CHUNKS = (16, 48, 64, 80, 128, 208, 1024)
BWD_ROWS = (2, 127, 128, 129, 3073, 6144, 6145, 12287)
BWD_SLABS = ((4, 4), (12, 20), (36, 68), (16, 100), (64, 512))


def all_cases():
    cs = []
    S = 'one_launch_tiles'
    cs += [case(S, 'block', 2, 16, 64, ('fwd', 1, False), sub='2'), case(S, 'block', 63, 16, 64, ('fwd', 1, False)),
           case(S, 'block', 64, 32, 64, ('fwd', 1, False)), case(S, 'block', 65, 48, 128, ('fwd', 1, False)),
           case(S, 'block', 1000, 80, 64, ('fwd', 1, False)), case(S, 'block', 4033, 16, 64, ('fwd', 1, False)),
           case(S, 'block', 1024, 16, 512, ('fwd', 2, False)), case(S, 'block', 961, 64, 512, ('fwd', 2, False)),
           case(S, 'block', 1024, 16, 1024, ('fwd', 4, False), ('fallback', '1')), case(S, 'block', 4096, 144, 256, ('fwd', 4, False)),
           case(S, 'block', 1000, 80, 64, ('fwd', 1, False), slope=1.0), case(S, 'block', 1024, 16, 1024, ('fwd', 4, False), slope=1.0)]
    cs += [case(S, 'block', 130, ci, 64, ('fwd', 1, False)) for ci in K_CHUNKS]
    S = 'tiled_forward'
    # (bias=False is make_inputs' default: as a keyword it only enters `build`'s seed -- the draw without it leaves dW below 1e-3 of dgamma
    # at 2 x 4 x 4 and `prepare` refuses it)
    cs += [case(S, 'block', 2, 4, 4, ('tiled', False), sub='2', bias=False), case(S, 'block', 33, 12, 20, ('tiled', False)),
           case(S, 'block', 100, 36, 100, ('tiled', False)), case(S, 'block', 4097, 16, 64, ('tiled', False)),
           case(S, 'block', 8160, 32, 128, ('tiled', False)), case(S, 'block', 8161, 32, 128, ('tiled', True)),
           case(S, 'block', 4100, 64, 256, ('tiled', True)), case(S, 'block', 6529, 16, 160, ('tiled', True))]
    S = 'fused_backward'
    sums = {2: '1', 127: '1', 128: '1', 129: '2..24', 3073: '25..48', 6144: '25..48', 6145: 'long', 12287: 'long'}
    cs += [case(S, 'block', m, 16, 64, ('sums', sums[m]), ('pro', False), sub='2' if m == 2 else None) for m in BWD_ROWS]
    cs += [case(S, 'block', 300, ci, co, ('sums', '2..24'), ('pro', False)) for ci, co in BWD_SLABS]
    cs += [case(S, 'block', 8161, 128, 32, ('pro', True)), case(S, 'block', 8161, 128, 32, ('pro', True), fork=True, galias=True),
           case(S, 'block', 12287, 64, 512, ('pro', False), ('tiled', True), ('sums', 'long'), fork=True, galias=True),
           case(S, 'block', 300, 36, 68, ('pro', False), fork=True, galias=True),
           case(S, 'chain', 3073, 64, 128, ('pro', False), ('fwd', 1, True), cj=16, galias=True, j_slope=0.3),
           case(S, 'chain', 8161, 128, 32, ('pro', True), ('tiled', True), cj=32, galias=True, j_slope=0.01),
           case(S, 'chain', 300, 36, 68, ('pro', False), cj=12, j_slope=0.3)]
    S = 'fallback_backward'
    cs += [case(S, 'block', 1024, 16, 1024, ('fallback', '1'), ('fwd', 4, False)), case(S, 'block', 2048, 16, 576, ('fallback', '3'), ('fwd', 4, False)),
           case(S, 'block', 1000, 16, 64, ('fallback', '1'), ('fwd', 1, False), want_dx=False),
           case(S, 'block', 3073, 16, 64, ('fallback', 'stream'), ('fwd', 1, False), want_dx=False),
           case(S, 'block', 4096, 16, 256, ('fallback', 'stream'), ('fwd', 4, False), want_dx=False),
           case(S, 'block', 6145, 36, 100, ('fallback', 'stream'), ('tiled', False), want_dx=False)]
    S = 'join'
    cs += [case(S, 'join', 1000, 80, 64, ('fwd', 1, True), slope=0.1), case(S, 'join', 1000, 80, 64, ('fwd', 1, True), slope=1.0),
           case(S, 'join', 1024, 16, 512, ('fwd', 2, True), slope=0.1), case(S, 'join', 4096, 16, 256, ('fwd', 4, True), slope=0.1),
           case(S, 'join', 4100, 64, 256, ('tiled', True), slope=0.1), case(S, 'join', 33, 12, 20, ('tiled', False), slope=0.1),
           case(S, 'join', 33, 12, 20, ('tiled', False), slope=1.0)]
    return cs


def label(c):
    return '%s-%dx%dx%d%s' % (c['kind'], c['m'], c['ci'], c['co'], ''.join('-%s=%s' % (k, v) for k, v in c['kw'].items()))


def cases_of(site):
    return [c for c in all_cases() if c['site'] == site]


def forms_of(c, cap):
    kw = c['kw']
    f = layer_forms(c['m'], c['ci'], c['co'], cap, c['kind'] == 'join', kw.get('want_dx', True) or c['kind'] == 'chain')
    if c['kind'] == 'chain':
        f |= layer_forms(c['m'], kw['cj'], c['ci'], cap, True)
    if c['site'] == 'fused_backward':
        f |= {('entry', 'one'), ('entry', 'two')}
    elif any(x[0] == 'pro' for x in f):
        f.add(('entry', 'one'))
    return f


@functools.lru_cache(maxsize=2)
def prepared(i):
    """(inputs, r32, r64) of case i of all_cases(), computed once and left unchanged."""
    with torch_seed():
        inp = build(all_cases()[i])
    r32, r64 = prepare(inp)
    return inp, r32, r64


def check_case(c, tag=''):
    i = all_cases().index(c)
    inp, r32, r64 = prepared(i)
    forms = forms_of(c, capacity())
    for w in c['what']:
        assert w in forms, (label(c), w, sorted(forms, key=str))
    got, names = run(inp)
    judge(c['key'], got, r32, r64, tag)
    gridsync_is_clean()
    return got, names


# group cases: blocks (m, ci, co, slope, fork, alias gradient), shared (blocks 0 and 1 on one tensor), cj (a fused join with a mask in
# front of the shared tensor)
GROUPS = {
    'two': dict(blocks=[(640, 64, 64, 0.1, False, False), (2560, 32, 128, 1.0, False, False)]),
    'three': dict(blocks=[(640, 64, 64, 0.1, False, False), (8161, 128, 32, 0.1, False, False), (33, 12, 20, 1.0, False, False)]),
    'four': dict(blocks=[(640, 64, 64, 0.1, False, False), (2560, 32, 128, 0.1, True, True), (8161, 32, 128, 1.0, False, False),
                         (33, 12, 20, 0.1, False, False)]),
    'shared': dict(blocks=[(300, 64, 64, 0.1, True, True), (300, 64, 32, 1.0, False, False), (100, 36, 100, 0.1, False, False)], shared=True),
    'shared_masked': dict(blocks=[(300, 64, 64, 0.1, True, True), (300, 64, 32, 1.0, False, False)], shared=True, cj=16),
}


def conditioned(r64):
    """`prepare`'s no-cancellation assertion on a result set put together here."""
    for group in KINDS + (None,):
        size = {k: float(v.abs().max()) for k, v in r64.items() if not k.startswith('_')
                and (k in group if group else not any(k in g for g in KINDS))}
        for k, s in size.items():
            assert s > 1e-3 * max(size.values()), '%s: max|ref64| %.3e against %.3e in its case: change the inputs' % (k, s, max(size.values()))


@functools.lru_cache(maxsize=None)
def group_prepared(name):
    """(inputs per block, r32 per block, r64 per block) of a group: every block through block_reference.  shared: the input gradient of
    the shared tensor is the sum of both blocks' (recorded with block 0; block 1 then has none).  cj: block 0 is the chain join ->
    block, block 1 reads the join's output, and its input gradient reaches the join as one more alias gradient of the chain."""
    g = GROUPS[name]
    rng = seed(77, len(name), *[v for b in g['blocks'] for v in b[:3]])
    inps = []
    for i, (m, ci, co, slope, fork, ga) in enumerate(g['blocks']):
        if g.get('cj') and i == 0:
            inps.append(make_inputs('chain', rng, m, ci, co, slope=slope, cj=g['cj'], galias=ga, j_slope=0.3))
        else:
            inps.append(make_inputs('block', rng, m, ci, co, slope=slope, fork=fork, galias=ga))
    if g.get('shared') and not g.get('cj'):
        inps[1]['x'] = inps[0]['x']
    refs = {}
    if g.get('cj'):
        nudge(inps[0])
        for dtype in (torch.float64, torch.float32):
            inps[1]['x'] = block_reference(inps[0], dtype)['j_out']
            if dtype == torch.float64:
                nudge(inps[1])                                      # beta of block 1, on the float64 join output
                prepare(dict(inps[1]))                              # (its assertions)
            r1 = block_reference(inps[1], dtype)
            r0 = block_reference(dict(inps[0], galias=inps[0]['galias'].to(dtype) + r1.pop('dx')), dtype)
            refs[dtype] = [r0, r1]
        prepare(dict(inps[0]))
        inps[1]['x'] = None                                         # (the device reads the join's output)
    else:
        pairs = [prepare(inp) for inp in inps]
        refs = {torch.float32: [p[0] for p in pairs], torch.float64: [p[1] for p in pairs]}
        if g.get('shared'):
            for r in refs.values():
                r[0]['dx'] = r[0]['dx'] + r[1].pop('dx')
    for r in refs[torch.float64]:
        assert r['_pre_min'] >= TAU
        conditioned(r)
    return inps, refs[torch.float32], refs[torch.float64]


def group_forms(name, cap):
    g = GROUPS[name]
    f = {('group', len(g['blocks'])), ('entry', 'one')}
    for m, ci, co, _, _, _ in g['blocks']:
        f |= layer_forms(m, ci, co, cap, group=True)
    if g.get('cj'):
        f |= layer_forms(g['blocks'][0][0], g['cj'], g['blocks'][0][1], cap, True)
    return f


def run_group(name):
    """The group on the device through ops.mlp_group: (results per block, entries called)."""
    from crfconv_amd import ops
    g = GROUPS[name]
    inps = group_prepared(name)[0]
    shared, cj = bool(g.get('shared')), g.get('cj')
    P = lambda v: torch.nn.Parameter(dev(v))
    names, got = [], [dict() for _ in inps]
    Ws = [P(inp['W']) for inp in inps]
    bns = [device_bn(inp, '') for inp in inps]
    with recorded(names):
        if cj:
            c0 = inps[0]
            J = dict(x=dev(c0['x']).requires_grad_(True), skip=dev(c0['skip']).requires_grad_(True), j_W=P(c0['j_W']))
            bnj = device_bn(c0, 'j_')
            mask = ops.JoinMask()
            poison(tuple(c0['skip'].shape), tuple(c0['skip'].shape))
            hs = ops.mlp_block_join(J['x'], J['j_W'], bnj, J['skip'], c0['j_slope'], mask=mask)
            assert NODES['join'] in graph_nodes(hs)
            xs = [hs, hs]
            got[0]['j_out'] = hs.detach().cpu()
        else:
            xs = [dev(inp['x']).requires_grad_(True) for inp in inps]
            if shared:
                xs[1] = xs[0]
        for inp in inps:
            poison(tuple(inp['gout'].shape), tuple(inp['gout'].shape))
        res = ops.mlp_group([(x, W, bn, inp['slope'], bool(b[4])) for x, W, bn, inp, b in zip(xs, Ws, bns, inps, g['blocks'])], shared=shared,
                            input_mask=mask if cj else None)
        assert res is not None, 'the group node refused the blocks'
        outs, grads = [], []
        for i, (r, inp, b) in enumerate(zip(res, inps, g['blocks'])):
            o, alias = r if b[4] else (r, None)
            nodes = graph_nodes(o)
            assert '_MLPSmallGroupBackward' in nodes and not any(n.startswith('_MLPBlock') for n in nodes), nodes
            assert cj or not any(n in nodes for n in NODES.values()), nodes
            got[i]['out'] = o.detach().cpu()
            outs.append(o)
            grads.append(dev(inp['gout']))
            if b[5]:
                assert alias is not xs[i]
                outs.append(alias)
                grads.append(dev(inp['galias']))
        if cj:
            assert mask.folded and mask.slope == inps[0]['j_slope']
        for inp in inps:
            poison(tuple(inp['x'].shape) if inp['x'] is not None else (1,), tuple(inp['gout'].shape), tuple(inp['W'].shape))
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    for i, (W, bn) in enumerate(zip(Ws, bns)):
        got[i].update(dW=W.grad.cpu(), dgamma=bn.weight.grad.cpu(), dbeta=bn.bias.grad.cpu(), rm=bn.running_mean.cpu(), rv=bn.running_var.cpu())
        assert int(bn.num_batches_tracked) == 1
        if not cj and not (shared and i == 1):
            got[i]['dx'] = xs[i].grad.cpu()
    if cj:
        got[0].update(dx=J['x'].grad.cpu(), dskip=J['skip'].grad.cpu(), j_dW=J['j_W'].grad.cpu(), j_dgamma=bnj.weight.grad.cpu(),
                      j_dbeta=bnj.bias.grad.cpu(), j_rm=bnj.running_mean.cpu(), j_rv=bnj.running_var.cpu())
    return got, names


# ------------------------------------------------------------------ 0: the union of the cases
def every_reached(cap):
    forms = set()
    for c in all_cases():
        forms |= forms_of(c, cap)
    for name in GROUPS:
        forms |= group_forms(name, cap)
    for ci, co in REGIME_WIDTHS:
        forms |= layer_forms(333, ci, co, cap) | {('entry', 'one')}
    return forms


def test_every_form_is_reached():
    """The cases of this file reach EVERY form of FORMS: TCO 1, 2, 4 of the one-launch forward without and with the join, the tiled
    forward and the PRO product on narrow and wide tiles, tile sums with ntile = 1, 2..24, 25..48 and with tile_rows > 128, both
    backward entries, the fallback through bn_small<1>, bn_small<3> and the streaming reduce, groups of 2, 3 and 4.  The capacity is
    the library's own answer, a positive multiple of 64.  No launch."""
    cap = capacity()
    assert cap > 0 and cap % 64 == 0
    forms = every_reached(cap)
    assert forms == FORMS, (sorted(FORMS - forms, key=str), sorted(forms - FORMS, key=str))
    k = constants()
    assert k['BT_MAXTILES'] == 48 and k['BT_ROUND'] == 24 and k['GG_MAX'] == 4 and max(len(g['blocks']) for g in GROUPS.values()) == k['GG_MAX']
    from crfconv_amd import _lib
    lib = _lib.load()
    for c in all_cases():                                       # the restatements against the library's own answers
        for m, ci, co in [(c['m'], c['ci'], c['co'])] + ([(c['m'], c['kw']['cj'], c['ci'])] if c['kind'] == 'chain' else []):
            assert lib.crfconv_mlp_small_supported(m, ci, co) == int(sm_shape_ok(m, ci, co) and sm_tco(m, co, cap) > 0), (m, ci, co)
            assert lib.crfconv_mlp_small_backward_supported(m, ci, co) == int(bwd_fused_ok(m, ci, co)), (m, ci, co)
            assert lib.crfconv_gemm_stat_records(m) == stat_records(m)
    # Row counts with M % 32 in 1 .. 16 leave the last 16-row record group of the tiled product empty
    assert sum(1 for c in cases_of('tiled_forward') if 1 <= c['m'] % 32 <= 16) >= 2


# ------------------------------------------------------------------ 1: the one-launch forward
@pytest.mark.parametrize('c', cases_of('one_launch_tiles'), ids=label)
def test_one_launch_tiles(c):
    """crfconv_mlp_small_forward (crfconv_gemm_stats does not run) in its three tile widths: TCO 1 at M = 2, 63, 64, 65, 1000 and 4033
    (64 row blocks, the last with one row: its wavefronts 1-3 publish n = 0 records, which the fold must skip), TCO 2 at Co = 512 with
    16 row blocks (961: the last with one row), TCO 4 at 1024 x 16 x 1024 (its backward is the fallback: Co > GM_PRO_MAXK) and 4096 x 144
    x 256 (all 64 row blocks in the coefficient fold, three K chunks with a tail of 16); K chunks at M = 130 with Ci = 16, 48, 64, 80,
    128, 208, 1024 (one chunk partial, full, two with a tail, ..., sixteen); slopes 1.0 and 0.1 at a TCO 1 and a TCO 4 shape.  The
    barrier words are zero afterwards.  Bounds and CPU e32: BOUNDS['one_launch_tiles'], ['one_launch_tiles/2']."""
    k = constants()
    if c['m'] == 4033:
        assert cdiv(c['m'], k['SM_ROWS']) == k['SM_MAX_ROWS'] // k['SM_ROWS'] and c['m'] % k['SM_ROWS'] == 1
    if c['m'] == 130:
        assert cdiv(c['ci'], k['SM_KC']) in (1, 2, 4, 16) and (c['ci'] % k['SM_KC'] != 0) == (c['ci'] in (16, 48, 80, 208))
    got, names = check_case(c)
    assert 'crfconv_mlp_small_forward' in names and 'crfconv_gemm_stats' not in names


# ------------------------------------------------------------------ 2: the tiled forward
@pytest.mark.parametrize('c', cases_of('tiled_forward'), ids=label)
def test_tiled_forward(c):
    """crfconv_gemm_stats + crfconv_bn_apply_from_records (crfconv_mlp_small_forward does not run).  Narrow 32 x 32 tiles: 2 x 4 x 4, 33 x
    12 x 20 and 100 x 36 x 100 (widths the one-launch kernel does not take; partial tiles in both directions), 4097 x 16 x 64 (the first
    row count past the one-launch limit), 8160 x 32 x 128 (255 x 4 = 1020 tiles: the last narrow shape).  Wide 32 x 64 tiles: 8161 x 32 x
    128 (1024 tiles, a one-row last tile), 4100 x 64 x 256, 6529 x 16 x 160 (205 x 5 = 1025: a column tail of 32 inside a 64-wide
    tile).  M % 32 in 1 .. 16 (2, 33, 100, 4097, 8161, 4100, 6529) leaves the last 16-row record group empty.  Bounds and CPU e32:
    BOUNDS['tiled_forward'], ['tiled_forward/2']."""
    k = constants()
    if (c['m'], c['co']) in ((8160, 128), (8161, 128)):
        assert cdiv(c['m'], 32) * cdiv(c['co'], 32) == k['WIDE_MIN_TILES'] - 4 * (c['m'] == 8160)
    if c['co'] == 160:
        assert gm_tile_plan(c['m'], c['co'])[1:] == (True, cdiv(c['m'], 32) * 3) and c['co'] % 64 == 32
    got, names = check_case(c)
    assert names.count('crfconv_gemm_stats') == 1 and names.count('crfconv_bn_apply_from_records') == 1 and 'crfconv_mlp_small_forward' not in names


# ------------------------------------------------------------------ 3: the fused backward, as one launch and as two
@pytest.mark.parametrize('c', cases_of('fused_backward'), ids=label)
def test_fused_backward(c, monkeypatch):
    """crfconv_mlp_small_backward_jobs_one_launch and, state.small_bwd_one_launch off, crfconv_mlp_small_backward_jobs: each judged against
    float64, and the two results bit-equal.  Tile plan at (Ci, Co) = (16, 64): M = 2, 127, 128 (one tile), 129 (two), 3073 (25 tiles:
    the second round of the last workgroup's sum), 6144 (48), 6145 (tile_rows 144: two trips of the row loop, 43 tiles), 12287 (tile_rows
    256).  Column slabs at M = 300: Co = 4, 20, 68, 100 (partial 64-channel slabs), 512 (eight).  The PRO product on wide tiles at 8161 x
    128 x 32, without and with the addend; on narrow tiles with the addend at 300 x 36 x 68 and 12287 x 64 x 512 (sixteen K chunks).  The
    masked epilogue through the public chain mlp_block_join(mask=) -> mlp_block(fork=True, input_mask=) at 3073 x 64 x 128 behind a
    one-launch join of 16 inputs, 8161 x 128 x 32 behind a tiled join of 32 inputs (wide tiles, addend and mask), and 300 x 36 x 68 without
    a second consumer; the join's slope is 0.3 or 0.01 beside the block's 0.1.  Bounds and CPU e32: BOUNDS['fused_backward'],
    ['fused_backward/2']."""
    from crfconv_amd import ops
    k = constants()
    plans = {3073: (25, 128), 6144: (48, 128), 6145: (43, 144), 12287: (48, 256), 129: (2, 128), 128: (1, 128)}
    if c['m'] in plans:
        assert bt_plan(c['m']) == plans[c['m']]
    if (c['ci'], c['co']) in BWD_SLABS:
        assert cdiv(c['co'], k['BT_CH']) == {4: 1, 20: 1, 68: 2, 100: 2, 512: 8}[c['co']] and (c['co'] % k['BT_CH'] != 0) == (c['co'] != 512)
    assert c['co'] <= k['PRO_MAXK'] and (c['co'] != 512 or cdiv(c['co'], k['GM_BK']) == 16)
    assert ops.state.small_bwd_one_launch
    got1, names1 = check_case(c, ' one launch')
    assert 'crfconv_mlp_small_backward_jobs_one_launch' in names1 and 'crfconv_mlp_small_backward_jobs' not in names1
    monkeypatch.setattr(ops.state, 'small_bwd_one_launch', False)
    got2, names2 = check_case(c, ' two launches')
    assert 'crfconv_mlp_small_backward_jobs' in names2 and 'crfconv_mlp_small_backward_jobs_one_launch' not in names2
    assert names1.count('crfconv_mlp_small_backward_jobs_one_launch') == names2.count('crfconv_mlp_small_backward_jobs') == (2 if c['kind'] == 'chain' else 1)
    for name in got1:
        assert torch.equal(got1[name], got2[name]), (name, float((got1[name] - got2[name]).abs().max()))


def eval_backward_reference(y, coef, gA, W, slope, dtype):
    """The BatchNorm(+LeakyReLU) backward with training = 0 on the float32 y and coef the kernel is given: dX = (a g1) W, dgamma and
    dbeta as in training."""
    co = W.shape[0]
    y, gA, W = y.to(dtype), gA.to(dtype), W.to(dtype)
    a, b, mu, rs = [coef[i * co:(i + 1) * co].to(dtype) for i in range(4)]
    pre = a * y + b
    g1 = gA * torch.where(pre > 0, torch.ones((), dtype=dtype), torch.full((), slope, dtype=dtype))
    gY = a * g1
    ones = torch.ones(1, y.shape[0], dtype=dtype)
    return dict(gY=gY, dx=rows_matmul(gY, W), dbeta=(ones @ g1)[0],
                dgamma=(ones @ (g1 * ((y - mu) * rs)))[0], _pre_min=float(pre.abs().min()))


@functools.lru_cache(maxsize=None)
def eval_backward_prepared():
    rng = seed(9, 300, 36, 68)
    inp = make_inputs('block', rng, 300, 36, 68)
    prepare(inp)
    y = rows_matmul(inp['x'].double(), inp['W'].double().t())
    mu, var = y.mean(0), y.var(0, unbiased=False)
    rs = 1.0 / torch.sqrt(var + EPS)
    a = inp['g'].double() * rs
    y32, coef = y.float(), torch.cat([a, inp['b'].double() - a * mu, mu, rs]).float().contiguous()
    r64, r32 = [eval_backward_reference(y32, coef, inp['gout'], inp['W'], 0.1, d) for d in (torch.float64, torch.float32)]
    assert r64['_pre_min'] >= TAU and r32['_pre_min'] >= 0.9 * TAU
    conditioned({k: v for k, v in r64.items() if k != 'gY'})
    return inp, y32, coef, r32, r64


def test_backward_entry_with_an_eval_mode_batchnorm():
    """One raw call of crfconv_mlp_small_backward with training = 0 at 300 x 36 x 68 (the wrappers never pass 0, so nothing else holds that
    branch of the last workgroup's finish): gY = a g1, dX = gY W, dgamma and dbeta as in training, against float64 on the same float32 y
    and coefficients.  Bounds and CPU e32: BOUNDS['eval_backward']."""
    from crfconv_amd import _lib, ops
    from crfconv_amd.graph import ptr, stream_ptr
    inp, y32, coef, r32, r64 = eval_backward_prepared()
    m, ci, co = 300, 36, 68
    assert bwd_fused_ok(m, ci, co) and bt_plan(m) == (3, 128) and not gm_wide(m, ci)
    gA, y, cf, W = dev(inp['gout']), dev(y32), dev(coef), dev(inp['W'])
    nb = _lib.load().crfconv_mlp_small_backward_workspace(m, co)
    poison((m, co), (m, ci), (co,), (co,))
    gY, dX = torch.empty((m, co), device=DEV), torch.empty((m, ci), device=DEV)
    dg, db, ws = torch.empty(co, device=DEV), torch.empty(co, device=DEV), torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.call('crfconv_mlp_small_backward', ptr(gA), ptr(y), ptr(cf), ptr(W), None, m, ci, co, 0, 0.1, ptr(gY), ptr(dX), ptr(dg), ptr(db),
              ptr(ws), nb, ops._mlp_ticket(DEV), stream_ptr())
    torch.cuda.synchronize()
    judge('eval_backward', dict(gY=gY.cpu(), dx=dX.cpu(), dgamma=dg.cpu(), dbeta=db.cpu()), r32, r64)
    gridsync_is_clean()


# ------------------------------------------------------------------ 4: the fallback backward
@pytest.mark.parametrize('c', cases_of('fallback_backward'), ids=label)
def test_fallback_backward(c):
    """crfconv_bn_backward (+ crfconv_gemm where dX is wanted) behind a one-launch or tiled forward; neither crfconv_mlp_small_backward
    entry runs.  Co > GM_PRO_MAXK: 1024 x 16 x 1024 (bn_small<1>: M <= 1024) and 2048 x 16 x 576 (bn_small<3>).  No dX wanted
    (requires_grad off for x): 1000 x 16 x 64 (bn_small<1>), 3073 x 16 x 64 and 4096 x 16 x 256 (past 3 x 1024 rows: the streaming
    reduce) and 6145 x 36 x 100 behind the tiled forward.  Bounds and CPU e32: BOUNDS['fallback_backward']."""
    got, names = check_case(c)
    assert names.count('crfconv_bn_backward') == 1 and not any(n.startswith('crfconv_mlp_small_backward') for n in names)
    assert ('crfconv_gemm' in names) == c['kw'].get('want_dx', True) and ('dx' in got) == c['kw'].get('want_dx', True)


# ------------------------------------------------------------------ 5: the join
@pytest.mark.parametrize('c', cases_of('join'), ids=label)
def test_join(c):
    """_MLPSmallJoin: the one-launch join (crfconv_mlp_small_forward_join) at 1000 x 80 x 64 (TCO 1, slopes 0.1 and 1.0), 1024 x 16 x 512
    (TCO 2) and 4096 x 16 x 256 (TCO 4); the tiled join (crfconv_bn_apply_from_records with skip) at 4100 x 64 x 256 (wide) and 33 x 12 x
    20 (slopes 0.1 and 1.0).  The pre-activation nudged away from 0 includes + skip; the gradient to skip is judged.  Bounds and CPU
    e32: BOUNDS['join']."""
    got, names = check_case(c)
    assert 'dskip' in got and names.count('crfconv_add_lrelu_backward') == 1


# ------------------------------------------------------------------ 6: the group node
@pytest.mark.parametrize('name', list(GROUPS))
def test_group(name):
    """ops.mlp_group: 2, 3 and 4 blocks of unequal shapes in one node (crfconv_gemm_stats_jobs and crfconv_bn_apply_from_records_jobs
    once each, one backward launch for all), narrow and wide jobs and differing M side by side -- 640 x 64 x 64, 2560 x 32 x 128, 8161 x
    32 x 128 (wide forward), 8161 x 128 x 32 (wide PRO product), 33 x 12 x 20 --, one block with fork=True and a gradient through its
    alias; shared=True with blocks 0 and 1 on one tensor (its gradient is the sum of both blocks' input gradients: crfconv_add_lrelu
    at slope 1); shared=True with input_mask behind a fused join and block 0 forked (crfconv_add_mask: the reference takes the sum through
    the join, whose dskip, dx, dW, dgamma, dbeta are judged).  Each block against its own block_reference.  Bounds and CPU e32:
    BOUNDS['group']."""
    g = GROUPS[name]
    inps, r32, r64 = group_prepared(name)
    forms = group_forms(name, capacity())
    assert ('group', len(inps)) in forms
    if name in ('three', 'four'):
        assert {('tiled', False), ('pro', False)} <= forms and (('pro', True) in forms) == (name == 'three') and (('tiled', True) in forms) == (name == 'four')
    got, names = run_group(name)
    for i in range(len(inps)):
        judge('group', got[i], r32[i], r64[i], ' block %d' % i)
    assert names.count('crfconv_gemm_stats_jobs') == 1 and names.count('crfconv_bn_apply_from_records_jobs') == 1
    assert names.count('crfconv_mlp_small_backward_jobs_one_launch') == (2 if g.get('cj') else 1)
    assert names.count('crfconv_add_mask') == (1 if g.get('cj') else 0)
    assert names.count('crfconv_add_lrelu') == (1 if g.get('shared') and not g.get('cj') else 0)
    no = {'crfconv_mlp_small_forward', 'crfconv_gemm_stats', 'crfconv_bn_apply_from_records', 'crfconv_mlp_small_backward_jobs', 'crfconv_bn_backward',
          'crfconv_gemm', 'crfconv_add_lrelu_backward'} | set(NEVER)
    assert not no & set(names), sorted(no & set(names))
    assert ('crfconv_mlp_small_forward_join' in names) == bool(g.get('cj'))
    gridsync_is_clean()


# ------------------------------------------------------------------ 7: input regimes
REGIME_WIDTHS = [(32, 64), (16, 32)]                           # at M = 333: the one-launch forward (TCO 1), the tiled forward


@pytest.mark.parametrize('regime', REGIMES)
def test_regimes(regime):
    """test_gpu_mlp_stream's three regimes (x with mean 100 and sigma 1, an upstream gradient of size 1e-5 with column means near 0, a
    column of y constant up to 1e-3) at M = 333 on the one-launch forward (32 -> 64) and on the tiled one (16 -> 32), both with the
    fused backward.  Bounds and CPU e32: BOUNDS['regimes/<regime>']."""
    assert ('fwd', 1, False) in layer_forms(333, 32, 64, capacity()) and ('tiled', False) in layer_forms(333, 16, 32, capacity())
    for ci, co in REGIME_WIDTHS:
        inp = regime_inputs(regime, ci, co)
        r32, r64 = prepare(inp)
        got, names = run(inp)
        judge('regimes/' + regime, got, r32, r64)
        gridsync_is_clean()


# ------------------------------------------------------------------ the CPU column of BOUNDS
def cpu_profile():
    """The float32 restatement of every case against the float64 one, on the CPU: prints, per (site, tensor), the largest e32 and the bound
    it gives (10 x, rounded up to one digit, at least 1e-6), and checks e32 against BOUNDS where BOUNDS has the pair."""
    import math
    worst, n = {}, 0

    def take(key, r32, r64):
        for k in r64:
            if not k.startswith('_'):
                e32 = errors(r32[k], r32[k], r64[k])[1]
                worst.setdefault(key, {})[k] = max(worst.get(key, {}).get(k, 0.0), e32)
    for i, c in enumerate(all_cases()):
        _, r32, r64 = prepared(i)
        take(c['key'], r32, r64)
        n += 1
    for name in GROUPS:
        _, r32, r64 = group_prepared(name)
        for a, b in zip(r32, r64):
            take('group', a, b)
        n += 1
    take('eval_backward', *eval_backward_prepared()[3:])
    for r in REGIMES:
        for ci, co in REGIME_WIDTHS:
            take('regimes/' + r, *prepare(regime_inputs(r, ci, co)))
            n += 2
    print('%d cases' % (n + 1))
    for key, d in worst.items():
        row = []
        for k, e32 in d.items():
            mag = 10.0 ** math.floor(math.log10(10.0 * e32)) if e32 > 0 else 1e-6
            b = max(math.ceil(10.0 * e32 / mag - 1e-9) * mag, 1e-6)
            row.append('%s=(%.0e, %.1e, None)' % (k, b, e32))
            if key in BOUNDS and k in BOUNDS[key]:
                assert e32 <= BOUNDS[key][k][0], (key, k, e32)
        print("    '%s': dict(%s)," % (key, ', '.join(row)))
    cap = 512                                                   # 256 compute units x 2 resident workgroups: what `capacity` finds on the MI355X
    forms = every_reached(cap)
    print('forms at a capacity of %d: %s' % (cap, 'all of FORMS' if forms == FORMS else 'missing %s, beyond %s' % (sorted(FORMS - forms, key=str),
                                                                                                                  sorted(forms - FORMS, key=str))))
    for c in all_cases():
        for w in c['what']:
            assert w in forms_of(c, cap), (label(c), w)


if __name__ == '__main__':
    cpu_profile()
