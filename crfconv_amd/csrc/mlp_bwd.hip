// The fused backward of one MLP block, Linear -> BatchNorm -> LeakyReLU, in two passes over the activations (the derivation
// stands above mlp_channel_part): the streaming pass mlp_bwd_p1_kernel, its finalize, the batched end-of-pass dW launches
// (mlp_dw_jobs_kernel, and the form that carries the CRF matrices' backward slabs of crf_matrices_body.hpp), and the dX product,
// which is linear_fwd_kernel<.., PRO = true> of linear_fwd.hpp -- this unit instantiates those forms.
// The narrow blocks of a fine-level CRF layer also run as JOBS -- up to four independent blocks per launch, each job its own single launch's
// workgroups laid end to end (mlp_bwd_p1_jobs_kernel here, linear_fwd_jobs_kernel<true> of linear_fwd.hpp; crfconv_mlp_backward_jobs).
#include "common.hpp"
#include "gridsync.hpp"
#include "wgrad_body.hpp"
#include "crf_matrices_body.hpp"
#include "linear_fwd.hpp"

namespace crf {

// ====================================================================== backward of Linear -> BatchNorm -> LeakyReLU
// (models/common.py:34-40, training mode) in TWO passes over the activations instead of four.  With
//   g1 = gA * lrelu'(a y + b),   yh = (y - mean) rstd,   dbeta = sum g1,   dgamma = sum g1 yh,
//   gY = a (g1 - dbeta / M - yh dgamma / M),   dX = gY W,   dW = gY^T X
// the weight gradient expands to   dW = diag(a) [ G1^T X - (dbeta / M) (1^T X) - diag(dgamma / M) Yh^T X ]:
// G1^T X, Yh^T X, 1^T X, sum g1 and sum g1 yh are all plain row reductions, so ONE streaming pass over (gA, Y, X)
// produces every partial (mlp_bwd_p1_kernel: two MFMA accumulator sets sharing the X fragment); a small finalize turns
// them into dgamma, dbeta, dW and the per-channel coefficients of gY; and dX = gY W is one more pass in which gY is
// formed in registers from (gA, Y) while loading the operand (linear_fwd_kernel<.., true>).  The step-by-step form
// (bn_bwd_reduce -> finalize -> bn_bwd_apply -> dX -> wgrad) reads or writes nine [M, C] arrays; this one six, with
// three launches instead of five, and gY never reaches memory.  (Two launches where the last workgroup of the first pass does the
// finalize's channel part: crfconv_mlp_backward's ticket.)

// dgamma, dbeta of channel c and the coefficients of  gY = alpha * lrelu'(a y + b) * gA + bet * y + del  (bcoef [5][Co] =
// a | b | alpha | bet | del) from the two channel sums s1 = sum g1, s2 = sum g1 yh
__device__ __forceinline__ void mlp_channel_part(int c, double s1, double s2, const float* __restrict__ coef, int64_t M, int Co,
                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ bcoef) {
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
    const double a = coef[c], mu = coef[2 * Co + c], rs = coef[3 * Co + c];
    const double c2 = s1 / (double)M, c3 = s2 / (double)M;
    bcoef[c] = coef[c];
    bcoef[Co + c] = coef[Co + c];
    bcoef[2 * Co + c] = (float)a;
    bcoef[3 * Co + c] = (float)(-a * c3 * rs);
    bcoef[4 * Co + c] = (float)(-a * c2 + a * c3 * rs * mu);
}

// Where the last workgroup of the pass keeps its 5 WG_BLOCK doubles (10 KB) of channel sums: inside s_red, the cross-wave reduction buffer
// of TCO TCI 4 KB (everybody has left it by then), when that is large enough; else in an array of their own (s_own).
template <int TCO, int TCI>
constexpr bool P1_ALIAS = TCO * TCI >= 3;

template <int TCO, int TCI>
__global__ __launch_bounds__(WG_BLOCK) void mlp_bwd_p1_kernel(const float* __restrict__ GA, const float* __restrict__ Y,
                                                              const float* __restrict__ X,
                                                              const float* __restrict__ X2, int split /*X = [X | X2] at column split (X2 may be null)*/,
                                                              const float* __restrict__ coef /*[4][Co]: a, b, mean, rstd*/,
                                                              float slope, int64_t M, int Co, int Ci, int rows_per_block,
                                                              float* __restrict__ PA /*[nblk][Co][Ci]*/,
                                                              float* __restrict__ PB /*[nblk][Co][Ci]*/,
                                                              float* __restrict__ PG /*[nblk][2][Co]*/,
                                                              float* __restrict__ PX /*[nblk][Ci]*/,
                                                              unsigned* __restrict__ ticket /*null: mlp_bwd_finalize_kernel does the channel part*/,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ bcoef) {
    __shared__ __attribute__((aligned(16))) float s_red[WG_WAVES][TCO * TCI * 256];
    __shared__ float s_v[WG_WAVES][(2 * TCO + TCI) * 16];
    __shared__ double s_own[P1_ALIAS<TCO, TCI> ? 1 : 5 * WG_BLOCK];
    __shared__ int s_flag;
#define P1_BX blockIdx.x
#define P1_BY blockIdx.y
#define P1_BZ blockIdx.z
#define P1_NBX gridDim.x
#define P1_LAST last_workgroup(ticket, gridDim.x * gridDim.y * gridDim.z, &s_flag)
#include "mlp_bwd_p1_body.inc"
#undef P1_BX
#undef P1_BY
#undef P1_BZ
#undef P1_NBX
#undef P1_LAST
}

// The same statements (mlp_bwd_p1_body.inc, the one home of them) as a device function of the workgroup's coordinates (bx, by, bz) in a grid
// of (nbx, nby, nbz), on LDS that the caller owns: a job's own coordinates in mlp_bwd_p1_jobs_kernel, and the last workgroup counted among
// the JOB's workgroups.  The kernel and this function both INCLUDE the text; neither calls the other: through a call the kernel's register
// counts move (profiles/r31_stream_groups.md), while the included text compiles to the code the kernel's own statements did
// (profiles/r32_shared_body.md).  s_own: 5 WG_BLOCK doubles for the last workgroup's sums where they do not go inside s_red (P1_ALIAS); it
// may lie inside the caller's larger reduction buffer -- everybody has left that by then.
template <int TCO, int TCI>
__device__ __forceinline__ void mlp_bwd_p1_body(const float* __restrict__ GA, const float* __restrict__ Y, const float* __restrict__ X,
                                                const float* __restrict__ X2, int split, const float* __restrict__ coef, float slope, int64_t M,
                                                int Co, int Ci, int rows_per_block, float* __restrict__ PA, float* __restrict__ PB,
                                                float* __restrict__ PG, float* __restrict__ PX, unsigned* __restrict__ ticket,
                                                float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ bcoef,
                                                const unsigned bx, const unsigned by, const unsigned bz, const unsigned nbx, const unsigned nby,
                                                const unsigned nbz, float (&s_red)[WG_WAVES][TCO * TCI * 256],
                                                float (&s_v)[WG_WAVES][(2 * TCO + TCI) * 16], double* s_own, int& s_flag) {
#define P1_BX bx
#define P1_BY by
#define P1_BZ bz
#define P1_NBX nbx
#define P1_LAST last_workgroup_of(ticket, nbx * nby * nbz, &s_flag, bx + nbx * (by + nby * bz))
#include "mlp_bwd_p1_body.inc"
#undef P1_BX
#undef P1_BY
#undef P1_BZ
#undef P1_NBX
#undef P1_LAST
}

// The pass of up to LFJ_MAX INDEPENDENT blocks in one launch: the jobs' own grids laid end to end (job j's workgroup (bx, by, bz) is
// workgroup blk_base[j] + bx + nbx (by + nby bz)), each with its own workspace, its own block of LW_TICKET_WORDS ticket words and its own
// last workgroup, which counts among the job's nbx nby nbz workgroups (last_workgroup_of).  Narrow outputs only: TCO = 1 (Co <= 16).
struct MlpP1Jobs {                                       // (slots at or past njobs are never read)
    const float* GA[LFJ_MAX]; const float* Y[LFJ_MAX]; const float* X[LFJ_MAX]; const float* coef[LFJ_MAX];
    float* PA[LFJ_MAX]; float* PB[LFJ_MAX]; float* PG[LFJ_MAX]; float* PX[LFJ_MAX];
    float* dgamma[LFJ_MAX]; float* dbeta[LFJ_MAX]; float* bcoef[LFJ_MAX];
    long long M[LFJ_MAX];
    int Co[LFJ_MAX], Ci[LFJ_MAX], rows_per_block[LFJ_MAX], nbx[LFJ_MAX], nbz[LFJ_MAX], tci[LFJ_MAX];
    float slope[LFJ_MAX];
    int blk_base[LFJ_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(WG_BLOCK) void mlp_bwd_p1_jobs_kernel(const MlpP1Jobs t, unsigned* __restrict__ tickets) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blockIdx.x) ++j;
    const unsigned local = blockIdx.x - (unsigned)t.blk_base[j];
    const unsigned nbx = (unsigned)uni(t.nbx[j]), nbz = (unsigned)uni(t.nbz[j]);
    const unsigned bx = (unsigned)uni((int)(local % nbx)), bz = (unsigned)uni((int)(local / nbx));      // nby = 1: one 16-channel output slab
    // one allocation for the widest form; the narrower forms' sums for the last workgroup go inside it as the wide form's do
    __shared__ __attribute__((aligned(16))) float s_red[WG_WAVES * 4 * 256];
    __shared__ float s_v[WG_WAVES * (2 + 4) * 16];
    __shared__ int s_flag;
    static_assert(sizeof(s_red) >= sizeof(double) * 5 * WG_BLOCK, "the last workgroup's sums fit the reduction buffer");
    unsigned* ticket = uni(tickets) + j * LW_TICKET_WORDS;
#define P1J(TCI) mlp_bwd_p1_body<1, TCI>(uni(t.GA[j]), uni(t.Y[j]), uni(t.X[j]), nullptr, 0, uni(t.coef[j]), uni(t.slope[j]), (int64_t)uni(t.M[j]), uni(t.Co[j]), \
                                        uni(t.Ci[j]), uni(t.rows_per_block[j]), uni(t.PA[j]), uni(t.PB[j]), uni(t.PG[j]), uni(t.PX[j]), ticket, uni(t.dgamma[j]), \
                                        uni(t.dbeta[j]), uni(t.bcoef[j]), bx, 0u, bz, nbx, 1u, nbz, *reinterpret_cast<float (*)[WG_WAVES][TCI * 256]>(s_red), \
                                        *reinterpret_cast<float (*)[WG_WAVES][(2 + TCI) * 16]>(s_v), reinterpret_cast<double*>(s_red), s_flag)
    const int tci = uni(t.tci[j]);
    if (tci == 1) P1J(1);
    else if (tci == 2) P1J(2);
    else P1J(4);
#undef P1J
}

// dW slots [64 block, 64 block + 64) of one MLP block's backward from its partial slabs (see mlp_bwd_finalize_kernel): shared by
// the per-layer finalize launch and the batched launch over all layers of a backward pass (mlp_dw_jobs_kernel).
constexpr int MF_BLOCK = 1024, MF_WAVES = MF_BLOCK / WAVE;
__device__ __forceinline__ void mlp_dw_slots(const float* __restrict__ PA, const float* __restrict__ PB,
                                             const float* __restrict__ PG, const float* __restrict__ PX, int nblk,
                                             const float* __restrict__ coef, int64_t M, int Co, int Ci, int block,
                                             float* __restrict__ dW) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // 64 slots per workgroup; the sixteen wavefronts split the slabs (b = w, w + 16, ..), four slabs of each of the five
    // streams in flight per lane: a 512-slab reduction is eight dependent round trips (the 256-thread form
    // measured 16.5 us per layer, more than the pass that produced the slabs)
    __shared__ float s_part[MF_WAVES][5][64];
    const int nslots = Co * Ci;
    const int slot = block * 64 + lane;
    const bool ok = slot < nslots;
    const int sl = ok ? slot : nslots - 1;
    const int co = sl / Ci, ci = sl - co * Ci;
    float a0 = 0.f, b0 = 0.f, x0 = 0.f, g1 = 0.f, g2 = 0.f;
    // four slabs of each stream in flight (20 loads per lane; eight spill at the 128-register budget of a 1024-thread block)
    const int64_t sa = (int64_t)MF_WAVES * Co * Ci, sx = (int64_t)MF_WAVES * Ci, sg = (int64_t)MF_WAVES * 2 * Co;
    const float* pa = PA + ((int64_t)w * Co + co) * Ci + ci;
    const float* pb = PB + ((int64_t)w * Co + co) * Ci + ci;
    const float* px = PX + (int64_t)w * Ci + ci;
    const float* pg = PG + (int64_t)w * 2 * Co + co;
#pragma unroll 1
    for (int b = w; b < nblk; b += 4 * MF_WAVES) {
        float va[4], vb[4], vx[4], vg[4], vh[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = b + MF_WAVES * u < nblk;
            va[u] = in ? pa[u * sa] : 0.f;
            vb[u] = in ? pb[u * sa] : 0.f;
            vx[u] = in ? px[u * sx] : 0.f;
            vg[u] = in ? pg[u * sg] : 0.f;
            vh[u] = in ? pg[u * sg + Co] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a0 += va[u]; b0 += vb[u]; x0 += vx[u]; g1 += vg[u]; g2 += vh[u]; }
        pa += 4 * sa; pb += 4 * sa; px += 4 * sx; pg += 4 * sg;
    }
    s_part[w][0][lane] = a0; s_part[w][1][lane] = b0; s_part[w][2][lane] = x0;
    s_part[w][3][lane] = g1; s_part[w][4][lane] = g2;
    __syncthreads();
    if (w == 0 && ok) {
        double A = 0.0, B = 0.0, Xs = 0.0, G1 = 0.0, G2 = 0.0;
        for (int k = 0; k < MF_WAVES; ++k) {
            A += s_part[k][0][lane]; B += s_part[k][1][lane]; Xs += s_part[k][2][lane];
            G1 += s_part[k][3][lane]; G2 += s_part[k][4][lane];
        }
        const double a = coef[co], c2 = G1 / (double)M, c3 = G2 / (double)M;
        dW[slot] = (float)(a * (A - c2 * Xs - c3 * B));
    }
}

// Finalize of the pass above, ONE launch of two kinds of workgroups:
//   blockIdx.x <  nw : 64 slots (co, ci) of dW = a [ sum A - c2 sum sx - c3 sum B ],  c2 = dbeta / M, c3 = dgamma / M
//                      (each workgroup re-derives c2 / c3 of the one or two co rows it touches: no ordering between the
//                      two kinds of workgroups is needed)
//   blockIdx.x >= nw : four channels each: dgamma, dbeta and the coefficients of
//                      gY = alpha * lrelu'(a y + b) * gA + bet * y + del   (bcoef [5][Co] = a | b | alpha | bet | del)
__global__ __launch_bounds__(MF_BLOCK) void mlp_bwd_finalize_kernel(const float* __restrict__ PA, const float* __restrict__ PB,
                                                                    const float* __restrict__ PG, const float* __restrict__ PX,
                                                                    int nblk, const float* __restrict__ coef, int64_t M, int Co,
                                                                    int Ci, int nw, float* __restrict__ dW,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                    float* __restrict__ bcoef) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x >= nw) {                               // one wavefront per channel
        const int c = ((int)blockIdx.x - nw) * MF_WAVES + w;
        if (c >= Co) return;
        double s1 = 0.0, s2 = 0.0;
        // eight slabs of both sums in flight per lane (nblk <= 512: ONE round trip; the rolled loop was eight dependent ones --
        // this launch sits between the two passes of every MLP block's backward)
        for (int b0 = lane; b0 < nblk; b0 += 8 * WAVE) {
            float v1[8], v2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int b = b0 + u * WAVE;
                const bool in = b < nblk;
                v1[u] = in ? PG[((int64_t)b * 2 + 0) * Co + c] : 0.f;
                v2[u] = in ? PG[((int64_t)b * 2 + 1) * Co + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { s1 += (double)v1[u]; s2 += (double)v2[u]; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, WAVE);
            s2 += __shfl_xor(s2, o, WAVE);
        }
        if (lane == 0) mlp_channel_part(c, s1, s2, coef, M, Co, dgamma, dbeta, bcoef);
        return;
    }
    mlp_dw_slots(PA, PB, PG, PX, nblk, coef, M, Co, Ci, (int)blockIdx.x, dW);
}

// The dW parts of ALL MLP blocks of a backward pass in ONE launch: nothing inside the pass reads a weight gradient, so the
// per-layer finalize launch only does its channel part (dgamma, dbeta, the dX coefficients) and the slab reductions --
// 32 launches of ~8 dependent round trips each -- run side by side at the end.  group_begin = prefix sum of ceil(Co Ci / 64).
constexpr int MDW_MAX = 40;
struct MlpDwTable {
    const float* PA[MDW_MAX];
    const float* PB[MDW_MAX];
    const float* PG[MDW_MAX];
    const float* PX[MDW_MAX];
    const float* coef[MDW_MAX];
    float* dW[MDW_MAX];
    long long M[MDW_MAX];
    int nblk[MDW_MAX], Co[MDW_MAX], Ci[MDW_MAX];
    int group_begin[MDW_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(MF_BLOCK) void mlp_dw_jobs_kernel(const MlpDwTable t) {
    const int g = blockIdx.x;
    int lo = 0, hi = t.njobs;                          // largest j with group_begin[j] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.group_begin[mid] <= g) lo = mid; else hi = mid;
    }
    mlp_dw_slots(t.PA[lo], t.PB[lo], t.PG[lo], t.PX[lo], t.nblk[lo], t.coef[lo], (int64_t)t.M[lo], t.Co[lo], t.Ci[lo],
                 g - t.group_begin[lo], t.dW[lo]);
}

// mlp_dw_jobs_kernel CARRYING the slabs of crf_matrices_bwd_batched_kernel as its first n_side workgroups (round 6): both are
// end-of-pass parameter work that nothing waits for; on its own the matrices' backward is a 13 us chain of three dependent float64
// products on 15 workgroups.  A rider uses the first CMB_BLOCK threads of its (MF_BLOCK-thread) workgroup.
static_assert(MF_BLOCK >= CMB_BLOCK, "a rider fits the host's workgroup");
__global__ __launch_bounds__(MF_BLOCK) void mlp_dw_jobs_hosting_kernel(const MlpDwTable t, const CrfMatJobs j, const int n_side) {
    if ((int)blockIdx.x < n_side) {
        int b = 0;
        while (b + 1 < CM_MAX && (int)blockIdx.x >= j.slab_base[b + 1]) ++b;
        crf_matrices_bwd_slab(j.c[b], j.Q_in[b], j.gQ[b], j.gP[b], j.H[b], ((int)blockIdx.x - j.slab_base[b]) * CMB_ROWS, j.dc[b]);
        return;
    }
    const int g = (int)blockIdx.x - n_side;
    int lo = 0, hi = t.njobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.group_begin[mid] <= g) lo = mid; else hi = mid;
    }
    mlp_dw_slots(t.PA[lo], t.PB[lo], t.PG[lo], t.PX[lo], t.nblk[lo], t.coef[lo], (int64_t)t.M[lo], t.Co[lo], t.Ci[lo],
                 g - t.group_begin[lo], t.dW[lo]);
}

// ---------------------------------------------------------------------- host side: plans, workspace layout, entry points
struct MlpPlan {
    int tco, tci, gy, gz, nblk, rows_per_block;
};
static MlpPlan mlp_plan(int64_t M, int Co, int Ci) {
    MlpPlan p;
    const int t_co = (Co + 15) / 16, t_ci = (Ci + 15) / 16;
    p.tco = t_co >= 4 ? 4 : (t_co >= 2 ? 2 : 1);
    p.tci = t_ci >= 4 ? 4 : (t_ci >= 2 ? 2 : 1);
    if (p.tco * p.tci == 16) p.tci = 2;              // two accumulator sets: at most 8 tiles (64 registers) each
    p.gy = (t_co + p.tco - 1) / p.tco;
    p.gz = (t_ci + p.tci - 1) / p.tci;
#ifndef MLP_P1_TARGET_
#define MLP_P1_TARGET_ 512
#endif
    constexpr int target = MLP_P1_TARGET_;           // slices x column slabs per launch (256 / 1024 measured slower: DESIGN 9 C4)
    int64_t slices = target / ((int64_t)p.gy * p.gz);
    if (slices < 32) slices = 32;
    int64_t rows = (M + slices - 1) / slices;
    if (rows < 64) rows = 64;
    rows = (rows + 63) / 64 * 64;
    p.rows_per_block = (int)rows;
    p.nblk = (int)((M + rows - 1) / rows);
    return p;
}
static size_t mlp_ws_layout(int64_t M, int Co, int Ci, size_t off[5]) {
    const MlpPlan p = mlp_plan(M, Co, Ci);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    off[0] = o; o = up(o + sizeof(float) * (size_t)p.nblk * Co * Ci);      // PA
    off[1] = o; o = up(o + sizeof(float) * (size_t)p.nblk * Co * Ci);      // PB
    off[2] = o; o = up(o + sizeof(float) * (size_t)p.nblk * 2 * Co);       // PG
    off[3] = o; o = up(o + sizeof(float) * (size_t)p.nblk * Ci);           // PX
    off[4] = o; o = up(o + sizeof(float) * 5 * (size_t)Co);                // prologue coefficients
    return o;
}
}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_ticket_bytes(void) { return sizeof(unsigned) * crf::LW_TICKET_WORDS; }

extern "C" int crfconv_mlp_backward_supported(int64_t M, int Ci, int Co) {
    if (!(M > 0 && Co % 4 == 0 && Ci >= 1 && Co >= 4 && Co <= 1024 && Ci <= 1024)) return 0;
    // dX runs on linear_fwd_kernel<., true> with k = Co inputs and Ci outputs: its LDS must fit 64 KB
    return lf_lds_bytes(Co, Ci, true) <= 64 * 1024 ? 1 : 0;
}

extern "C" size_t crfconv_mlp_backward_workspace(int64_t M, int Ci, int Co) {
    if (M <= 0 || Co <= 0 || Ci <= 0) return 0;
    size_t off[5];
    return crf::mlp_ws_layout(M, Co, Ci, off) + 256;
}

static int mlp_backward_impl(const float* gA, const float* Y, const float* X, const float* Xb, int xsplit, const float* W,
                             const float* coef, float slope, int64_t M, int Ci, int Co, float* dX, float* dXb, float* dW,
                             float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, unsigned* ticket,
                             crf_stream_t stream, const float* dX_add = nullptr, const float* mask_ref = nullptr,
                             float mask_slope = 1.f) {
    CRF_REQUIRE(gA && Y && X && W && coef && dgamma && dbeta && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(mask_ref == nullptr || (dX_add != nullptr && dX != nullptr && Ci % 4 == 0 && Co % 4 == 0), CRF_ERR_ARG,
                "the masked dX takes an addend and widths that are multiples of 4 (Ci=%d Co=%d)", Ci, Co);
    CRF_REQUIRE(dX_add == nullptr || dXb == nullptr, CRF_ERR_ARG, "dX_add is for the one-operand form");
    CRF_REQUIRE(crfconv_mlp_backward_supported(M, Ci, Co) == 1, CRF_ERR_UNSUPPORTED, "shape M=%lld Ci=%d Co=%d not supported",
                (long long)M, Ci, Co);
    CRF_REQUIRE(workspace_bytes >= crfconv_mlp_backward_workspace(M, Ci, Co), CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = crf::as_stream(stream);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    size_t off[5];
    crf::mlp_ws_layout(M, Co, Ci, off);
    float* PA = reinterpret_cast<float*>(base + off[0]);
    float* PB = reinterpret_cast<float*>(base + off[1]);
    float* PG = reinterpret_cast<float*>(base + off[2]);
    float* PX = reinterpret_cast<float*>(base + off[3]);
    float* pro = reinterpret_cast<float*>(base + off[4]);
    const crf::MlpPlan p = crf::mlp_plan(M, Co, Ci);
    // the last workgroup of pass 1 does the channel part when its 2 Co sums fit one thread each in groups of whole quads
    if (!(2 * Co <= crf::WG_BLOCK && crf::WG_BLOCK % (Co / 2) == 0 && (int64_t)p.nblk * 2 * Co * 4 < ((int64_t)1 << 31))) ticket = nullptr;
    {
        const dim3 grid((unsigned)p.nblk, (unsigned)p.gy, (unsigned)p.gz), blk(crf::WG_BLOCK);
#define P1(TA, TB) hipLaunchKernelGGL((crf::mlp_bwd_p1_kernel<TA, TB>), grid, blk, 0, st, gA, Y, X, Xb, xsplit, coef, slope, M, Co, Ci, p.rows_per_block, PA, PB, PG, PX, ticket, dgamma, dbeta, pro)
        switch (p.tco * 10 + p.tci) {
            case 11: P1(1, 1); break;
            case 12: P1(1, 2); break;
            case 14: P1(1, 4); break;
            case 21: P1(2, 1); break;
            case 22: P1(2, 2); break;
            case 24: P1(2, 4); break;
            case 41: P1(4, 1); break;
            default: P1(4, 2); break;
        }
#undef P1
        CRF_LAUNCH_CHECK();
    }
    // dW == NULL: the channel part only; the caller finishes dW later from the workspace (crfconv_mlp_dw_jobs)
    const int nw = dW != nullptr ? (int)crf::cdiv((int64_t)Co * Ci, 64) : 0;
    const int nc = ticket != nullptr ? 0 : (Co + crf::MF_WAVES - 1) / crf::MF_WAVES;      // channel workgroups (none: done inside pass 1)
    if (nw + nc > 0) {
        hipLaunchKernelGGL(crf::mlp_bwd_finalize_kernel, dim3((unsigned)(nw + nc)), dim3(crf::MF_BLOCK), 0, st, PA, PB, PG, PX, p.nblk, coef, M, Co,
                           Ci, nw, dW, dgamma, dbeta, pro);
        CRF_LAUNCH_CHECK();
    }
    if (dX != nullptr) {
        // dX [M, Ci] = gY [M, Co] W [Co, Ci]: the forward kernel with k = Co, outputs = Ci, W read transposed
        crf::LfArgs a;
        a.X = gA; a.W = W; a.M = M; a.Ci = Co; a.Co = Ci; a.transpose_w = 1; a.Y = dX;
        a.Y2 = Y; a.pro = pro; a.slope = slope;
        a.Yb = dXb; a.ysplit = xsplit;
        a.addend = dX_add; a.mask_ref = mask_ref; a.mask_slope = mask_slope;
        return crf::lf_launch<true>(a, mask_ref != nullptr ? crf::EPI_ADD_MASK : (dX_add != nullptr ? crf::EPI_ADD : crf::EPI_NONE), stream);
    }
    return CRF_OK;
}

extern "C" int crfconv_mlp_backward(const float* gA, const float* Y, const float* X, const float* W, const float* coef,
                                    float slope, int64_t M, int Ci, int Co, float* dX, float* dW, float* dgamma,
                                    float* dbeta, void* workspace, size_t workspace_bytes, unsigned* ticket,
                                    crf_stream_t stream) {
    return mlp_backward_impl(gA, Y, X, nullptr, 0, W, coef, slope, M, Ci, Co, dX, nullptr, dW, dgamma, dbeta, workspace,
                             workspace_bytes, ticket, stream);
}

// dX = (the block's input gradient) + dX_add [M, Ci]: the block's input has a second consumer (the shortcut of a ResNet block)
// whose gradient is already known -- the sum autograd would form in a pass of its own is made while dX is written.
extern "C" int crfconv_mlp_backward_add(const float* gA, const float* Y, const float* X, const float* W, const float* coef,
                                        float slope, int64_t M, int Ci, int Co, const float* dX_add, float* dX, float* dW,
                                        float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                        unsigned* ticket, crf_stream_t stream) {
    CRF_REQUIRE(dX != nullptr || dX_add == nullptr, CRF_ERR_ARG, "dX_add without dX");
    return mlp_backward_impl(gA, Y, X, nullptr, 0, W, coef, slope, M, Ci, Co, dX, nullptr, dW, dgamma, dbeta, workspace,
                             workspace_bytes, ticket, stream, dX_add);
}

// The same with the LeakyReLU mask of the ResNet join that PRODUCED the block's input x folded in: dX = mask(gY W + dX_add; X, mask_slope),
// mask(v; ref, s) = ref > 0 ? v : s v -- what crfconv_add_lrelu_backward(dX, X, ...) would make of crfconv_mlp_backward_add's dX in a
// pass of its own (same float operations: bit-identical).  dX is then the join's g1.  Ci % 4 == 0.  dX_add == NULL (the alias had no
// gradient): the plain product, then that pass in place.
// crfconv_add_lrelu_backward lives in pool.hip; the header declares it.
extern "C" int crfconv_mlp_backward_add_mask(const float* gA, const float* Y, const float* X, const float* W, const float* coef,
                                             float slope, int64_t M, int Ci, int Co, const float* dX_add, float mask_slope, float* dX,
                                             float* dW, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                             unsigned* ticket, crf_stream_t stream) {
    CRF_REQUIRE(dX != nullptr && Ci % 4 == 0, CRF_ERR_ARG, "the masked form writes dX, Ci=%d a multiple of 4", Ci);
    if (dX_add == nullptr) {
        if (int rc = mlp_backward_impl(gA, Y, X, nullptr, 0, W, coef, slope, M, Ci, Co, dX, nullptr, dW, dgamma, dbeta, workspace,
                                       workspace_bytes, ticket, stream))
            return rc;
        return crfconv_add_lrelu_backward(dX, X, M * Ci, mask_slope, dX, stream);
    }
    return mlp_backward_impl(gA, Y, X, nullptr, 0, W, coef, slope, M, Ci, Co, dX, nullptr, dW, dgamma, dbeta, workspace,
                             workspace_bytes, ticket, stream, dX_add, X, mask_slope);
}

// The block's input was the column concatenation [Xa | Xb]: dXa [M, split], dXb [M, Ci - split] (both or neither NULL).
extern "C" int crfconv_mlp_backward_cat(const float* gA, const float* Y, const float* Xa, const float* Xb, int split,
                                        const float* W, const float* coef, float slope, int64_t M, int Ci, int Co,
                                        float* dXa, float* dXb, float* dW, float* dgamma, float* dbeta, void* workspace,
                                        size_t workspace_bytes, unsigned* ticket, crf_stream_t stream) {
    CRF_REQUIRE(Xb && split > 0 && split < Ci && split % 4 == 0 && Ci % 4 == 0 && ((dXa == nullptr) == (dXb == nullptr)),
                CRF_ERR_ARG, "two-operand form: split=%d Ci=%d must be multiples of 4, dXa / dXb both or neither", split, Ci);
    return mlp_backward_impl(gA, Y, Xa, Xb, split, W, coef, slope, M, Ci, Co, dXa, dXb, dW, dgamma, dbeta, workspace,
                             workspace_bytes, ticket, stream);
}

// crfconv_mlp_backward_add for up to 4 INDEPENDENT blocks in TWO launches in all: pass 1 of every job (mlp_bwd_p1_jobs_kernel), then
// every wanted dX product (linear_fwd_jobs_kernel<true>) -- per job the workgroups, summation orders, workspace slabs and results of its
// own call.  Narrow blocks: Co in {4, 8, 16} (one output slab in pass 1, one k chunk in dX, the channel part by the last workgroup).
extern "C" int crfconv_mlp_backward_p1_jobs_supported(int64_t M, int Ci, int Co) {
    if (crfconv_mlp_backward_supported(M, Ci, Co) != 1) return 0;
    const crf::MlpPlan p = crf::mlp_plan(M, Co, Ci);
    return (p.tco == 1 && p.gy == 1 && 2 * Co <= crf::WG_BLOCK && crf::WG_BLOCK % (Co / 2) == 0 &&
            (int64_t)p.nblk * 2 * Co * 4 < ((int64_t)1 << 31)) ? 1 : 0;
}
extern "C" int crfconv_mlp_backward_dx_jobs_supported(int64_t M, int Ci, int Co) {
    crf::LfArgs a;
    a.M = M; a.Ci = Co; a.Co = Ci; a.transpose_w = 1;
    return crf::lf_job_ok<true>(a, crf::EPI_NONE) ? 1 : 0;
}

extern "C" int crfconv_mlp_backward_jobs(const crf_mlp_stream_bwd_job* jobs, int njobs, unsigned* tickets, crf_stream_t stream) {
    CRF_REQUIRE(jobs && tickets && njobs >= 1 && njobs <= crf::LFJ_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d) and their ticket words", crf::LFJ_MAX, njobs);
    hipStream_t st = crf::as_stream(stream);
    crf::MlpP1Jobs t{};
    crf::LfArgs dx[crf::LFJ_MAX];
    int epi[crf::LFJ_MAX], ndx = 0;
    int64_t blocks = 0;
    for (int j = 0; j < njobs; ++j) {
        const crf_mlp_stream_bwd_job& b = jobs[j];
        CRF_REQUIRE(b.gA && b.Y && b.X && b.W && b.coef && b.dgamma && b.dbeta && b.workspace, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(b.dX != nullptr || b.dX_add == nullptr, CRF_ERR_ARG, "job %d: dX_add without dX", j);
        CRF_REQUIRE(crfconv_mlp_backward_p1_jobs_supported(b.M, b.Ci, b.Co) == 1 && crfconv_mlp_backward_dx_jobs_supported(b.M, b.Ci, b.Co) == 1,
                    CRF_ERR_UNSUPPORTED, "job %d: shape M=%lld Ci=%d Co=%d is not a narrow row-streaming block", j, (long long)b.M, b.Ci, b.Co);
        CRF_REQUIRE(b.workspace_bytes >= crfconv_mlp_backward_workspace(b.M, b.Ci, b.Co), CRF_ERR_WORKSPACE, "job %d: workspace too small", j);
        char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(b.workspace) + 255) & ~(uintptr_t)255);
        size_t off[5];
        crf::mlp_ws_layout(b.M, b.Co, b.Ci, off);
        const crf::MlpPlan p = crf::mlp_plan(b.M, b.Co, b.Ci);
        t.GA[j] = b.gA; t.Y[j] = b.Y; t.X[j] = b.X; t.coef[j] = b.coef;
        t.PA[j] = reinterpret_cast<float*>(base + off[0]); t.PB[j] = reinterpret_cast<float*>(base + off[1]);
        t.PG[j] = reinterpret_cast<float*>(base + off[2]); t.PX[j] = reinterpret_cast<float*>(base + off[3]);
        t.bcoef[j] = reinterpret_cast<float*>(base + off[4]);
        t.dgamma[j] = b.dgamma; t.dbeta[j] = b.dbeta; t.M[j] = (long long)b.M; t.Co[j] = b.Co; t.Ci[j] = b.Ci;
        t.rows_per_block[j] = p.rows_per_block; t.nbx[j] = p.nblk; t.nbz[j] = p.gz; t.tci[j] = p.tci; t.slope[j] = b.slope;
        t.blk_base[j] = (int)blocks;
        blocks += (int64_t)p.nblk * p.gz;
        if (b.dX != nullptr) {
            crf::LfArgs& a = dx[ndx];
            a.X = b.gA; a.W = b.W; a.M = b.M; a.Ci = b.Co; a.Co = b.Ci; a.transpose_w = 1; a.Y = b.dX;
            a.Y2 = b.Y; a.pro = t.bcoef[j]; a.slope = b.slope; a.addend = b.dX_add;
            epi[ndx++] = b.dX_add != nullptr ? crf::EPI_ADD : crf::EPI_NONE;
        }
    }
    for (int j = njobs; j <= crf::LFJ_MAX; ++j) t.blk_base[j] = (int)blocks;
    t.njobs = njobs;
    hipLaunchKernelGGL(crf::mlp_bwd_p1_jobs_kernel, dim3((unsigned)blocks), dim3(crf::WG_BLOCK), 0, st, t, tickets);
    CRF_LAUNCH_CHECK();
    for (int j = 0; j < njobs; ++j) {              // a weight gradient wanted now (not deferred to crfconv_mlp_dw_jobs): that job's dW workgroups
        const crf_mlp_stream_bwd_job& b = jobs[j];
        if (b.dW == nullptr) continue;
        const int nw = (int)crf::cdiv((int64_t)b.Co * b.Ci, 64);
        hipLaunchKernelGGL(crf::mlp_bwd_finalize_kernel, dim3((unsigned)nw), dim3(crf::MF_BLOCK), 0, st, t.PA[j], t.PB[j], t.PG[j], t.PX[j], t.nbx[j], b.coef,
                           b.M, b.Co, b.Ci, nw, b.dW, b.dgamma, b.dbeta, t.bcoef[j]);
        CRF_LAUNCH_CHECK();
    }
    return ndx > 0 ? crf::lf_launch_jobs<true>(dx, epi, ndx, stream) : CRF_OK;
}

// dW of any number of MLP blocks whose crfconv_mlp_backward(_add / _cat) call was given dW = NULL, from the workspaces those
// calls left behind (untouched since), in ONE launch.
static int mlp_dw_jobs_impl(const crf_mlp_dw_job* jobs, int njobs, const crf::CrfMatJobs* side, int nside, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = crf::as_stream(stream);
    for (int j0 = 0; j0 < njobs; j0 += crf::MDW_MAX) {
        crf::MlpDwTable t;
        const int n = njobs - j0 < crf::MDW_MAX ? njobs - j0 : crf::MDW_MAX;
        int64_t total = 0;
        for (int j = 0; j < crf::MDW_MAX; ++j) {
            const crf_mlp_dw_job& jb = jobs[j0 + (j < n ? j : 0)];
            if (j < n) {
                CRF_REQUIRE(jb.workspace && jb.coef && jb.dW, CRF_ERR_ARG, "job %d: null pointer", j0 + j);
                CRF_REQUIRE(crfconv_mlp_backward_supported(jb.M, jb.Ci, jb.Co) == 1, CRF_ERR_UNSUPPORTED,
                            "job %d: shape M=%lld Ci=%d Co=%d not supported", j0 + j, (long long)jb.M, jb.Ci, jb.Co);
            }
            const char* base = reinterpret_cast<const char*>((reinterpret_cast<uintptr_t>(jb.workspace) + 255) & ~(uintptr_t)255);
            size_t off[5];
            crf::mlp_ws_layout(jb.M, jb.Co, jb.Ci, off);
            t.PA[j] = reinterpret_cast<const float*>(base + off[0]);
            t.PB[j] = reinterpret_cast<const float*>(base + off[1]);
            t.PG[j] = reinterpret_cast<const float*>(base + off[2]);
            t.PX[j] = reinterpret_cast<const float*>(base + off[3]);
            t.coef[j] = jb.coef;
            t.dW[j] = jb.dW;
            t.M[j] = (long long)jb.M;
            t.nblk[j] = crf::mlp_plan(jb.M, jb.Co, jb.Ci).nblk;
            t.Co[j] = jb.Co;
            t.Ci[j] = jb.Ci;
            t.group_begin[j] = (int)total;
            if (j < n) total += crf::cdiv((int64_t)jb.Co * jb.Ci, 64);
            CRF_REQUIRE(total < ((int64_t)1 << 30), CRF_ERR_ARG, "too many slots in one batch");
        }
        t.group_begin[crf::MDW_MAX] = (int)total;
        t.njobs = n;
        if (side != nullptr && j0 == 0)
            hipLaunchKernelGGL(crf::mlp_dw_jobs_hosting_kernel, dim3((unsigned)(total + nside)), dim3(crf::MF_BLOCK), 0, st, t, *side, nside);
        else
            hipLaunchKernelGGL(crf::mlp_dw_jobs_kernel, dim3((unsigned)total), dim3(crf::MF_BLOCK), 0, st, t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}
extern "C" int crfconv_mlp_dw_jobs(const crf_mlp_dw_job* jobs, int njobs, crf_stream_t stream) {
    return mlp_dw_jobs_impl(jobs, njobs, nullptr, 0, stream);
}
// crfconv_mlp_dw_jobs whose (first) launch also CARRIES crfconv_crf_matrices_backward_batched(c, Q, gQ, gP, H, n, dc) as its first
// workgroups: results of both are those of the two separate calls.
extern "C" int crfconv_mlp_dw_jobs_hosting(const crf_mlp_dw_job* jobs, int njobs, const float* const* c, const float* const* Q,
                                           const float* const* gQ, const float* const* gP, const int* H, int n, float* const* dc,
                                           crf_stream_t stream) {
    CRF_REQUIRE(njobs >= 1, CRF_ERR_ARG, "a hosting launch needs at least one job of its own (got %d)", njobs);
    crf::CrfMatJobs j;
    int nslab = 0;
    if (int rc = crf_matrices_bwd_jobs(c, Q, gQ, gP, H, n, dc, j, nslab)) return rc;
    return mlp_dw_jobs_impl(jobs, njobs, &j, nslab, stream);
}
