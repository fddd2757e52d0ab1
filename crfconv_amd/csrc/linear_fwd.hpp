// linear_fwd_kernel, the row-streaming product of the per-point Linear layers, with its planning helpers and its ONE host launcher
// (lf_launch), shared by the two units that instantiate it: linear.hip (the forward forms, PRO = false) and mlp_bwd.hip (the dX
// product of the fused MLP backward, PRO = true).
#pragma once
#include "common.hpp"
#include "stream_jobs.h"
#include "uv_fold.hpp"

#include <type_traits>

namespace crf {

// ====================================================================== Y = X W^T (+ b) with BN statistics
// The per-point Linear layers at the fine levels: m = 10^4..10^5 rows, Ci, Co <= 128.  One wavefront owns 16 rows
// and all Co outputs; X rows are read ONCE as float4 (lane l: row l & 15, k = 16 c + 4 (l >> 4) + {0..3}), W sits in
// LDS (rows padded by 4 floats: conflict-free ds_read_b128), and each float4 pair feeds four
// v_mfma_f32_16x16x4_f32 steps (step s takes component s of every lane's float4: the k order inside a 16-chunk is
// permuted identically for both operands, which a sum does not notice).  Output tile D[co][row]: lane holds 4
// consecutive co of one row -> one float4 store.  Optional epilogue: per-block shifted sums / sums of squares of
// every output channel, so BatchNorm needs no separate statistics pass over Y.

#ifndef LF_BLOCK_
#define LF_BLOCK_ 256
#endif
constexpr int LF_BLOCK = LF_BLOCK_, LF_WAVES = LF_BLOCK / WAVE;

// PRO: the operand is not read but formed while loading (dX of the fused MLP backward): row r, channel k of
//   gY = alpha[k] * lrelu'(a[k] y + b[k]) * X[r][k] + bet[k] * Y2[r][k] + del[k]     (X = gA, Y2 = the Linear's output y)
// pro = [5][Ci] floats a | b | alpha | bet | del, staged in LDS behind the weight slab (Ci % 4 == 0 required).
// VEC4: Ci % 4 == 0 and Co % 4 == 0 -- every access is a 16-byte one and the element-wise tail code does not exist.  (With
// both forms in one kernel the compiler merges the float4 store into the four predicated dword stores of the tail path:
// 4x the store instructions and 3x the write requests, 983 k instead of 328 k per 21 MB -- TCP_TCC_WRITE_REQ.)
// EPI: 0 plain store; 1 (PRO) Y += addend; 2 (not PRO) dropout mask on Y.  Template forms, so that the common kernels keep their
// register budget (as run-time branches the two epilogues cost <2, false> and <4, true> one wavefront per SIMD each).
// 3 (PRO, VEC4) Y = mask(Y + addend; mask_ref, mask_slope), mask(v; ref, s) = ref > 0 ? v : s v -- lrelu_bwd_kernel's (pool.hip): the
// dX of a block whose input is the output of a ResNet join is handed to that join with the join's LeakyReLU mask already applied.
// 4 (not PRO, VEC4, Ci <= 16; a PROLOGUE despite the parameter's name, which is the one free slot of the kernel's template list): the operand is the
// PointConv combine helper(U, V) of uv_fold.hpp, formed when the fragment is loaded (X = U, uv.V = V) and stored to uv.out by the same lane
// -- each row group is streamed by ONE workgroup per column group, the first column group stores; workgroup (0, 0) publishes a2 / b2 / aux2
// and advances BatchNorm-2's running statistics as uv_combine_kernel's workgroup 0 does.  lin_out of a fine-level ResNet block.
// 5 (not PRO; Co % 4 == 0): the eval-mode MLP block in the product's epilogue -- Y = lrelu(add_rn(fmaf(a, y, b), skip), slope) with
// pro = the BatchNorm's [>= 2][Co] coefficient rows a | b, addend = skip [M, Co] (or null: no residual) and slope (1: no activation):
// bn_apply_kernel's / bn_apply_add_kernel's arithmetic (bn.hip) on the accumulator instead of on a stored y.  No statistic records.
constexpr int EPI_NONE = 0, EPI_ADD = 1, EPI_DROPOUT = 2, EPI_ADD_MASK = 3, EPI_UV = 4, EPI_BN_ACT = 5;
// NCH > 0 (round 4; Ci <= 16 NCH, VEC4): the operand fragments of ALL k chunks of a row group are requested at once and those of
// the wavefront's NEXT row group before the current group's products (NCH <= LF_PF_MAX) -- the rolled loop (NCH = 0) pays one
// dependent memory round trip per chunk, eight per group at 128 inputs, with two to four wavefronts per SIMD to hide them.
#ifndef LF_PF_MAX_
#define LF_PF_MAX_ 4
#endif
template <int NCH>
constexpr bool PF = NCH > 0 && NCH <= LF_PF_MAX_;                 // next group's fragments in flight too
template <int TCO, bool PRO = false, bool VEC4 = true, int EPI = EPI_NONE, int NCH = 0>  // 16 * TCO output channels per block slab (blockIdx.y picks the slab)
__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                              const float* __restrict__ bias, int64_t M, int Ci, int Co,
                                                              int transpose_w, float* __restrict__ Y,
                                                              float* __restrict__ stat_partial /*[nblk][Co][4] or null*/,
                                                              const float* __restrict__ Y2 = nullptr,
                                                              const float* __restrict__ pro = nullptr, float slope = 1.f,
                                                              const float* __restrict__ Xb = nullptr, int xsplit = 0,
                                                              float* __restrict__ Yb = nullptr, int ysplit = 0,
                                                              const float* __restrict__ addend = nullptr,
                                                              const long long* __restrict__ drop_counter = nullptr,
                                                              unsigned long long drop_seed = 0ull, unsigned drop_threshold = 0u,
                                                              float drop_scale = 1.f,
                                                              const float* __restrict__ mask_ref = nullptr, float mask_slope = 1.f,
                                                              const UvFold uv = UvFold()) {
    extern __shared__ float sW[];                 // [16*TCO][Cip] (+ [5][Cik] prologue coefficients) (+ the output staging tiles)
#define LF_BX blockIdx.x
#define LF_BY blockIdx.y
#define LF_NBX gridDim.x
#include "linear_fwd_body.inc"
#undef LF_BX
#undef LF_BY
#undef LF_NBX
}

// The same statements (linear_fwd_body.inc, the one home of them) as a device function of the workgroup's coordinates (bx, by) in a grid of
// nbx row workgroups: a job's own coordinates and block count in linear_fwd_jobs_kernel, whose launch is the jobs' single launches laid end
// to end.  The kernel and this function both INCLUDE the text; neither calls the other: when the kernel called this function the register
// counts of 27 instantiations moved and two dX forms lost a wavefront per SIMD (profiles/r31_stream_groups.md), while the included text
// compiles to the code the kernel's own statements did (profiles/r32_shared_body.md).
template <int TCO, bool PRO, bool VEC4, int EPI, int NCH>
__device__ __forceinline__ void linear_fwd_body(const float* __restrict__ X, const float* __restrict__ W,
                                                const float* __restrict__ bias, int64_t M, int Ci, int Co,
                                                int transpose_w, float* __restrict__ Y,
                                                float* __restrict__ stat_partial /*[nblk][Co][4] or null*/,
                                                const float* __restrict__ Y2, const float* __restrict__ pro, float slope,
                                                const float* __restrict__ Xb, int xsplit, float* __restrict__ Yb, int ysplit,
                                                const float* __restrict__ addend, const long long* __restrict__ drop_counter,
                                                unsigned long long drop_seed, unsigned drop_threshold, float drop_scale,
                                                const float* __restrict__ mask_ref, float mask_slope, const UvFold& uv,
                                                const unsigned bx, const unsigned by, const unsigned nbx) {
    extern __shared__ float sW[];                 // (the launch's dynamic LDS: the largest of its jobs' sizes, lf_jobs_plan)
#define LF_BX bx
#define LF_BY by
#define LF_NBX nbx
#include "linear_fwd_body.inc"
#undef LF_BX
#undef LF_BY
#undef LF_NBX
}

static int lf_blocks(int64_t M) {
    constexpr int cap = 512;   // swept 128..2048 on the training step: 512 (two blocks per CU, half the statistic records of 1024) is the optimum
    int64_t nb = (M + 16 * LF_WAVES - 1) / (16 * LF_WAVES);           // 16 rows per wave and iteration; two blocks per CU keep
    if (nb > cap) nb = cap;               // enough 16-byte loads in flight; one statistics record per block
    return (int)(nb < 1 ? 1 : nb);
}

// Supported when a 16-channel weight slab fits LDS: 16 x (Ci rounded to 16 + 4) floats (+ prologue rows) <= 64 KB, i.e. Ci <= ~1000.
// Output tiles per workgroup and the dynamic LDS of linear_fwd_kernel for k = Ci inputs, Co outputs: weight slab
// [16 tco][Ci rounded to 16, + 4], the five prologue coefficient rows (dX form), the four output staging tiles (tco >= 2).
// 64 output channels per workgroup at most: the 128-channel form (tco = 8) needs 167 + 98 registers with the statistic
// accumulators, i.e. ONE wavefront per SIMD (measured 68 -> 49 us for 163840 x 32 -> 128; 5.85 -> 5.80 ms per step).  The kernel
// is therefore instantiated for tco = 1, 2 and 4 only (lf_launch).
static size_t lf_lds_bytes_at(int Ci, int tco, bool pro) {
    const size_t cip = (size_t)((Ci + 15) / 16) * 16 + 4, cik = cip - 4;
    size_t floats = 16 * (size_t)tco * cip;
    const size_t stats = (size_t)crf::LF_WAVES * 4 * 16 * (size_t)tco;   // the statistics epilogue reuses the slab as [waves][4][16 tco]
    if (floats < stats) floats = stats;
    if (pro) floats += 5 * cik;
    if (tco >= 2) floats += (size_t)crf::LF_WAVES * 16 * (16 * (size_t)tco + 4);
    return sizeof(float) * floats;
}
// Output tiles per workgroup: by Co, then halved until the slab of k = Ci inputs fits 64 KB (256 inputs: 32 channels per
// workgroup, 512: 16 -- the operand rows are then read once per column slab, from L2).
static int lf_tco(int Ci, int Co, bool pro) {
    constexpr int max_tco = 4;
    const int tiles = (Co + 15) / 16;
    int tco = tiles >= max_tco ? max_tco : (tiles >= 2 ? 2 : 1);
    while (tco > 1 && lf_lds_bytes_at(Ci, tco, pro) > 64 * 1024) tco >>= 1;
    return tco;
}
static size_t lf_lds_bytes(int Ci, int Co, bool pro) { return lf_lds_bytes_at(Ci, lf_tco(Ci, Co, pro), pro); }
// k chunks of the hoisted operand loop (linear_fwd_kernel<.., NCH>): Ci <= 128 in 16-byte pieces; else 0 = the rolled loop
static int lf_hoist_chunks(int Ci, bool vec4) {
    if (!vec4 || Ci > 128) return 0;
    const int n = (Ci + 15) / 16;
    return n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : 8));
}

// ---------------------------------------------------------------------- host side: one argument record, one launcher
struct LinearDropout {
    const long long* counter = nullptr;
    unsigned long long seed = 0ull;
    unsigned threshold = 0u;
    float scale = 1.f;
};

// the eval-mode block's epilogue (EPI_BN_ACT): coef = the BatchNorm's coefficient rows a | b, skip [M, Co] or null, slope (1: none)
struct LinearBnAct {
    const float* coef = nullptr;
    const float* skip = nullptr;
    float slope = 1.f;
};

// linear_fwd_kernel's arguments by name, with the kernel's defaults.  A caller fills what its form uses; lf_launch is the only place
// that lists them positionally.  (A record for the HOST: the kernel keeps its __restrict__ pointer parameters.)
struct LfArgs {                                                  // (grouped as the kernel's parameter list is)
    const float* X = nullptr; const float* W = nullptr;          // X [M, Ci] (PRO: gA; EPI_UV: U); W [Co, Ci], or [Ci, Co] with transpose_w
    const float* bias = nullptr; int64_t M = 0; int Ci = 0, Co = 0;
    int transpose_w = 0; float* Y = nullptr;
    float* stat_partial = nullptr;
    const float* Y2 = nullptr;                                   // PRO: the Linear's output y, the [5][Ci] coefficient rows, the LeakyReLU slope
    const float* pro = nullptr; float slope = 1.f;
    const float* Xb = nullptr; int xsplit = 0;                   // operand [X | Xb] split at column xsplit
    float* Yb = nullptr; int ysplit = 0;                         // output columns >= ysplit
    const float* addend = nullptr;                               // EPI_ADD, EPI_ADD_MASK
    LinearDropout drop;                                          // EPI_DROPOUT
    const float* mask_ref = nullptr; float mask_slope = 1.f;     // EPI_ADD_MASK
    LinearBnAct bn;                                              // EPI_BN_ACT: travels in the kernel's pro / slope / addend parameters
    UvFold uv;                                                   // EPI_UV
};

// The instantiations of linear_fwd_kernel that exist; lf_launch refuses every other combination.  TCO is 1, 2 or 4 (lf_tco).  The
// hoisted operand loop (NCH > 0) is the aligned forms', and the dropout epilogue keeps the rolled one.  dX (PRO): no epilogue or the
// addend, and addend + mask when aligned.  Forward: none, dropout, BatchNorm + activation, and the combine prologue on
// <2 | 4, false, true, EPI_UV, 1> alone.
template <int TCO, bool PRO, bool VEC4, int EPI, int NCH>
constexpr bool lf_form() {
    if (EPI == EPI_UV) return !PRO && VEC4 && TCO >= 2 && NCH == 1;
    if (NCH > 0 && (!VEC4 || EPI == EPI_DROPOUT)) return false;
    if (PRO) return EPI == EPI_NONE || EPI == EPI_ADD || (EPI == EPI_ADD_MASK && VEC4);
    return EPI == EPI_NONE || EPI == EPI_DROPOUT || EPI == EPI_BN_ACT;
}

// f(std::integral_constant<int, V>()) for the V among Vs that equals v (none: no call): a run-time value as a template argument
template <int... Vs, class F>
static void lf_pick(int v, F f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}

// The one launch of linear_fwd_kernel: output tiles per workgroup, alignment, hoisted chunks, grid and LDS are planned here, and the
// instantiation follows from them and the caller's epilogue (the caller has checked its own shapes).
template <bool PRO>
static int lf_launch(const LfArgs& a, int epi, crf_stream_t stream) {
    const int tiles = (a.Co + 15) / 16, tco = lf_tco(a.Ci, a.Co, PRO);
    const bool vec4 = (a.Ci % 4) == 0 && (a.Co % 4) == 0;
    const int nch = epi == EPI_DROPOUT ? 0 : lf_hoist_chunks(a.Ci, vec4);       // 1 / 2 / 4 / 8 chunks: the hoisted loop; 0: the rolled one
    const dim3 grid((unsigned)lf_blocks(a.M), (unsigned)((tiles + tco - 1) / tco)), blk(LF_BLOCK);
    const size_t lds = lf_lds_bytes_at(a.Ci, tco, PRO);
    hipStream_t st = as_stream(stream);
    bool launched = false;
    lf_pick<1, 2, 4>(tco, [&](auto T) { lf_pick<0, 1>(vec4, [&](auto V) {
    lf_pick<EPI_NONE, EPI_ADD, EPI_DROPOUT, EPI_ADD_MASK, EPI_UV, EPI_BN_ACT>(epi, [&](auto E) { lf_pick<0, 1, 2, 4, 8>(nch, [&](auto N) {
        constexpr int TCO = decltype(T)::value, EPI = decltype(E)::value, NCH = decltype(N)::value;
        constexpr bool VEC4 = decltype(V)::value != 0, BNA = EPI == EPI_BN_ACT;
        if constexpr (lf_form<TCO, PRO, VEC4, EPI, NCH>()) {
            hipLaunchKernelGGL((linear_fwd_kernel<TCO, PRO, VEC4, EPI, NCH>), grid, blk, lds, st, a.X, a.W, a.bias, a.M, a.Ci, a.Co,
                               a.transpose_w, a.Y, a.stat_partial, a.Y2, BNA ? a.bn.coef : a.pro, BNA ? a.bn.slope : a.slope, a.Xb,
                               a.xsplit, a.Yb, a.ysplit, BNA ? a.bn.skip : a.addend, a.drop.counter, a.drop.seed, a.drop.threshold,
                               a.drop.scale, a.mask_ref, a.mask_slope, a.uv);
            launched = true;
        }
    }); }); }); });
    CRF_REQUIRE(launched, CRF_ERR_UNSUPPORTED, "linear_fwd_kernel has no form pro=%d epi=%d for %d -> %d", (int)PRO, epi, a.Ci, a.Co);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// ---------------------------------------------------------------------- several INDEPENDENT products per launch
// Up to LFJ_MAX jobs whose single launches (lf_launch) are laid end to end in one grid: workgroup blk_base[j] + bx + nbx by of the launch
// is workgroup (bx, by) of job j's own grid of nbx = lf_blocks(M_j) row workgroups, and runs the instantiation that job's launch would --
// the same rows, summation order and statistic records.  A fine-level launch of these widths is a chain of dependent round trips on
// <= 512 workgroups of 36-76 registers: two of them side by side cost about the longer one.  Forms: the forward's <1, false, true, EPI_NONE,
// 1 | 2 | 4> (Co <= 16, Ci <= 64, one operand, no bias) and the dX product's <1 | 2 | 4, true, true, EPI_NONE | EPI_ADD, 1> (k <= 16).
constexpr int LFJ_MAX = 4;                               // (= GG_MAX of gemm_tile.hpp, BA_MAX of bn_records.hip: the group nodes' size)
struct LfJobs {                                          // (slots at or past njobs are never read)
    const float* X[LFJ_MAX]; const float* W[LFJ_MAX]; float* Y[LFJ_MAX]; float* stat[LFJ_MAX];
    const float* Y2[LFJ_MAX]; const float* pro[LFJ_MAX]; const float* addend[LFJ_MAX];
    long long M[LFJ_MAX];
    int Ci[LFJ_MAX], Co[LFJ_MAX], nbx[LFJ_MAX], form[LFJ_MAX];      // form: NCH (forward); 2 TCO + (addend != null) (dX)
    float slope[LFJ_MAX];
    int blk_base[LFJ_MAX + 1];
    int njobs;
};
// workgroup `blk` of the jobs' grids laid end to end (blockIdx.x in linear_fwd_jobs_kernel; behind the hosted tiles in linear.hip's
// linear_fwd_jobs_hosting_kernel)
template <bool PRO>
__device__ __forceinline__ void linear_fwd_jobs_block(const LfJobs& t, const unsigned blk) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blk) ++j;
    const unsigned local = blk - (unsigned)t.blk_base[j];
    const unsigned nbx = (unsigned)uni(t.nbx[j]);
    const unsigned bx = (unsigned)uni((int)(local % nbx)), by = (unsigned)uni((int)(local / nbx));
    const float* X = uni(t.X[j]); const float* W = uni(t.W[j]); float* Y = uni(t.Y[j]);
    const int64_t M = uni(t.M[j]);
    const int Ci = uni(t.Ci[j]), Co = uni(t.Co[j]), form = uni(t.form[j]);
    if constexpr (!PRO) {
        float* stat = uni(t.stat[j]);
#define LFJ_FWD(NCH) linear_fwd_body<1, false, true, EPI_NONE, NCH>(X, W, nullptr, M, Ci, Co, 0, Y, stat, nullptr, nullptr, 1.f, nullptr, 0, nullptr, 0, \
                                                                    nullptr, nullptr, 0ull, 0u, 1.f, nullptr, 1.f, UvFold(), bx, by, nbx)
        if (form == 1) LFJ_FWD(1);
        else if (form == 2) LFJ_FWD(2);
        else LFJ_FWD(4);
#undef LFJ_FWD
    } else {
        const float* Y2 = uni(t.Y2[j]); const float* pro = uni(t.pro[j]); const float* addend = uni(t.addend[j]);
        const float slope = uni(t.slope[j]);
#define LFJ_DX(TCO, EPI) linear_fwd_body<TCO, true, true, EPI, 1>(X, W, nullptr, M, Ci, Co, 1, Y, nullptr, Y2, pro, slope, nullptr, 0, nullptr, 0, addend, \
                                                                  nullptr, 0ull, 0u, 1.f, nullptr, 1.f, UvFold(), bx, by, nbx)
        switch (form) {
            case 2: LFJ_DX(1, EPI_NONE); break;
            case 3: LFJ_DX(1, EPI_ADD); break;
            case 4: LFJ_DX(2, EPI_NONE); break;
            case 5: LFJ_DX(2, EPI_ADD); break;
            case 8: LFJ_DX(4, EPI_NONE); break;
            default: LFJ_DX(4, EPI_ADD); break;
        }
#undef LFJ_DX
    }
}
template <bool PRO>
__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_jobs_kernel(const LfJobs t) {
    linear_fwd_jobs_block<PRO>(t, blockIdx.x);
}

// Whether linear_fwd_jobs_kernel<PRO> has the form lf_launch<PRO> would pick for this job (a: the arguments of its single launch)
template <bool PRO>
static bool lf_job_ok(const LfArgs& a, int epi) {
    if (a.M < 1 || a.Ci < 1 || a.Co < 1 || (a.Ci % 4) != 0 || (a.Co % 4) != 0) return false;
    if (a.bias != nullptr || a.Xb != nullptr || a.Yb != nullptr || a.mask_ref != nullptr) return false;
    if (lf_lds_bytes(a.Ci, a.Co, PRO) > 64 * 1024) return false;
    const int tco = lf_tco(a.Ci, a.Co, PRO), nch = lf_hoist_chunks(a.Ci, true);
    if (PRO) return a.transpose_w != 0 && nch == 1 && (epi == EPI_NONE || epi == EPI_ADD);
    return a.transpose_w == 0 && epi == EPI_NONE && tco == 1 && a.Co <= 16 && (nch == 1 || nch == 2 || nch == 4);
}

// The job table of one launch: per job the plan of lf_launch (row workgroups, column slabs, instantiation); dynamic LDS is the largest of
// the jobs' sizes (the body lays its slabs out from its own widths).  epi[j]: EPI_NONE, or EPI_ADD with a[j].addend.
template <bool PRO>
static int lf_jobs_plan(const LfArgs* a, const int* epi, int njobs, LfJobs& t, int64_t& blocks, size_t& lds) {
    CRF_REQUIRE(a && njobs >= 1 && njobs <= LFJ_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d)", LFJ_MAX, njobs);
    t = LfJobs{};
    blocks = 0;
    lds = 0;
    for (int j = 0; j < njobs; ++j) {
        const LfArgs& b = a[j];
        CRF_REQUIRE(lf_job_ok<PRO>(b, epi[j]), CRF_ERR_UNSUPPORTED, "job %d: linear_fwd_jobs_kernel has no form pro=%d epi=%d for %lld x %d -> %d", j,
                    (int)PRO, epi[j], (long long)b.M, b.Ci, b.Co);
        const int tiles = (b.Co + 15) / 16, tco = lf_tco(b.Ci, b.Co, PRO);
        t.X[j] = b.X; t.W[j] = b.W; t.Y[j] = b.Y; t.stat[j] = b.stat_partial; t.Y2[j] = b.Y2; t.pro[j] = b.pro;
        t.addend[j] = epi[j] == EPI_ADD ? b.addend : nullptr;
        t.M[j] = (long long)b.M; t.Ci[j] = b.Ci; t.Co[j] = b.Co; t.nbx[j] = lf_blocks(b.M); t.slope[j] = b.slope;
        t.form[j] = PRO ? 2 * tco + (epi[j] == EPI_ADD ? 1 : 0) : lf_hoist_chunks(b.Ci, true);
        t.blk_base[j] = (int)blocks;
        blocks += (int64_t)t.nbx[j] * ((tiles + tco - 1) / tco);
        const size_t need = lf_lds_bytes_at(b.Ci, tco, PRO);
        if (need > lds) lds = need;
    }
    for (int j = njobs; j <= LFJ_MAX; ++j) t.blk_base[j] = (int)blocks;
    t.njobs = njobs;
    return CRF_OK;
}
template <bool PRO>
static int lf_launch_jobs(const LfArgs* a, const int* epi, int njobs, crf_stream_t stream) {
    LfJobs t;
    int64_t blocks;
    size_t lds;
    if (int rc = lf_jobs_plan<PRO>(a, epi, njobs, t, blocks, lds)) return rc;
    hipLaunchKernelGGL((linear_fwd_jobs_kernel<PRO>), dim3((unsigned)blocks), dim3(LF_BLOCK), lds, as_stream(stream), t);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

}  // namespace crf
