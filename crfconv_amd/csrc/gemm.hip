// Small dense products of the per-point layers on the coarse levels:  C [M, N] = A [M, K] · B (+ bias [N]) (+ addend [M, N])
//
// The shapes the row-streaming kernels of linear_fwd.hpp do not take: the coarse-level forward (models/common.py:30,35 -- MLP.lin
// at 640 .. 10 240 rows, up to 512 channels) and every dX = gY · W of the MLP / ResNet-block backward (autograd of the same
// lines), plus the per-edge g_h1 = g_h2 · W2 of the wide PointConv layers (models/point_conv_big.py:45-47).  M is small
// (10^2 .. 10^5), K and N are 32 .. 512: a few hundred MFLOP each, bounded by dependent memory round trips and by how many
// wavefronts the grid gives the 1024 SIMDs, not by the matrix pipe.  The tile shape is picked per problem so that the grid covers
// the chip.
//
// The plain forms of the tile routine of gemm_tile.hpp: crfconv_gemm (bias / addend epilogue, any widths), crfconv_gemm_bn_act (the
// eval-mode BatchNorm + activation epilogue) and crfconv_gemm_jobs (several independent products in one launch).  The product with
// statistic records is gemm_stats.hip, the backward of the coarse MLP block mlp_small_bwd.hip.
#include "gemm_tile.hpp"

namespace crf {

template <int WM, int WN, int WR, int WC, bool BNK, bool VEC>
__global__ __launch_bounds__(GM_BLOCK) void gemm_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                        const float* __restrict__ bias, const float* __restrict__ addend,
                                                        int M, int N, int K, float* __restrict__ C) {
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<WM, WN, WR, WC, BNK, false>()];
    gemm_tile<WM, WN, WR, WC, BNK, VEC, false, false>(A, B, bias, addend, M, N, K, C, GemmPro(), nullptr, blockIdx.x, blockIdx.y, lds);
}

// the plain form with the BNACT epilogue (crfconv_gemm_bn_act): coef [>= 2][N] = a | b, skip [M, N] or null
template <int WM, int WN, int WR, int WC, bool BNK, bool VEC>
__global__ __launch_bounds__(GM_BLOCK) void gemm_bn_act_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                               const float* __restrict__ bias, const float* __restrict__ skip,
                                                               int M, int N, int K, float* __restrict__ C,
                                                               const float* __restrict__ coef, float slope) {
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<WM, WN, WR, WC, BNK, false>()];
    GemmPro pro;
    pro.coef = coef;
    pro.slope = slope;
    gemm_tile<WM, WN, WR, WC, BNK, VEC, false, false, false, true>(A, B, bias, skip, M, N, K, C, pro, nullptr, blockIdx.x, blockIdx.y, lds);
}

// SEVERAL products C_j = A_j B_j (B [K, N], aligned widths, 32 x 32 tiles) in one launch: the tiles of the jobs are laid end to
// end, a workgroup finds its job by a scan over the (<= 8) prefix entries -- crfconv_gemm_jobs, the g_h1 = g_h2 W2 products of all
// wide PointConv layers of a backward pass.
constexpr int GJ_MAX = 8;
struct GemmJobs {                                       // (slots at or past njobs are never read)
    const float* A[GJ_MAX]; const float* B[GJ_MAX]; float* C[GJ_MAX];
    int M[GJ_MAX], N[GJ_MAX], K[GJ_MAX], tiles_x[GJ_MAX];
    int tile_base[GJ_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(GM_BLOCK) void gemm_jobs_kernel(const GemmJobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.tile_base[j + 1] <= (int)blockIdx.x) ++j;
    const unsigned local = blockIdx.x - (unsigned)t.tile_base[j];
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<1, 1, 2, 2, false, false>()];
    gemm_tile<1, 1, 2, 2, false, true, false, false>(t.A[j], t.B[j], nullptr, nullptr, t.M[j], t.N[j], t.K[j], t.C[j], GemmPro(), nullptr,
                                                     local % (unsigned)t.tiles_x[j], local / (unsigned)t.tiles_x[j], lds);
}

// an instantiation of gemm_kernel / gemm_bn_act_kernel, as a value for gm_dispatch's callable
template <int WM_, int WN_, int WR_, int WC_, bool BNK_, bool VEC_>
struct GmForm {
    static constexpr int WM = WM_, WN = WN_, WR = WR_, WC = WC_;
    static constexpr bool BNK = BNK_, VEC = VEC_;
};

// tile shapes (rows x columns per workgroup): 0 = 64 x 64, 1 = 32 x 64, 2 = 64 x 32, 3 = 32 x 32 -- the largest that still gives the
// grid `min_blocks` workgroups.  Measured on the shapes of the training step (scratch/gemm_bench.py, graph replays): 32 x 32 is the
// fastest or within 0.5 us of it from 640 x 64 to 163 840 x 32 -- these launches are latency-bound, many short wavefronts win
static int gemm_shape(int64_t M, int N) {
    constexpr int min_blocks = 4096;
    auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * (int64_t)((N + bn - 1) / bn); };
    if (N > 32 && blocks(64, 64) >= min_blocks) return 0;
    if (N > 32 && blocks(32, 64) >= min_blocks) return 1;
    if (blocks(64, 32) >= min_blocks) return 2;
    return 3;
}

// The one place where (M, N), the storage order of B and the alignment pick an instantiation of the plain kernels:
// f(GmForm<WM, WN, WR, WC, BNK, VEC>{}, grid) for the shape of gemm_shape(M, N).  vec: 16-byte accesses.
template <class F>
static void gm_dispatch(int64_t M, int N, bool b_is_nk, bool vec, F&& f) {
    auto forms = [&](auto S) {                           // S: the shape (its BNK, VEC are not read)
        using T = decltype(S);
        const dim3 grid((unsigned)cdiv(M, 16 * T::WM * T::WR), (unsigned)cdiv(N, 16 * T::WN * T::WC));
        if (b_is_nk && vec) f(GmForm<T::WM, T::WN, T::WR, T::WC, true, true>{}, grid);
        else if (b_is_nk) f(GmForm<T::WM, T::WN, T::WR, T::WC, true, false>{}, grid);
        else if (vec) f(GmForm<T::WM, T::WN, T::WR, T::WC, false, true>{}, grid);
        else f(GmForm<T::WM, T::WN, T::WR, T::WC, false, false>{}, grid);
    };
    switch (gemm_shape(M, N)) {
        case 0: forms(GmForm<2, 2, 2, 2, false, false>{}); break;
        case 1: forms(GmForm<1, 2, 2, 2, false, false>{}); break;
        case 2: forms(GmForm<1, 2, 4, 1, false, false>{}); break;
        default: forms(GmForm<1, 1, 2, 2, false, false>{}); break;
    }
}

}  // namespace crf

// C_j [M_j, N_j] = A_j [M_j, K_j] B_j [K_j, N_j] for up to 8 products per launch (jobs: host array); N, K multiples of 4.  Same tiles
// and summation order as crfconv_gemm on each job.
extern "C" int crfconv_gemm_jobs(const crf_gemm_job* jobs, int njobs, void* stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = crf::as_stream(stream);
    for (int j0 = 0; j0 < njobs; j0 += crf::GJ_MAX) {
        crf::GemmJobs t{};
        const int n = njobs - j0 < crf::GJ_MAX ? njobs - j0 : crf::GJ_MAX;
        int64_t tiles = 0;
        for (int j = 0; j < n; ++j) {
            const crf_gemm_job& jb = jobs[j0 + j];
            CRF_REQUIRE(jb.A && jb.B && jb.C, CRF_ERR_ARG, "job %d: null pointer", j0 + j);
            CRF_REQUIRE(jb.M >= 1 && jb.M < ((int64_t)1 << 31) && jb.N >= 4 && jb.K >= 4 && jb.N % 4 == 0 && jb.K % 4 == 0, CRF_ERR_UNSUPPORTED,
                        "job %d: %lld x %d x %d (N, K multiples of 4)", j0 + j, (long long)jb.M, jb.N, jb.K);
            crf::GmTilePlan p;
            if (int rc = crf::gm_tile_plan(jb.M, jb.N, false, tiles, p)) return rc;
            t.A[j] = jb.A; t.B[j] = jb.B; t.C[j] = jb.C; t.M[j] = (int)jb.M; t.N[j] = jb.N; t.K[j] = jb.K;
            t.tiles_x[j] = p.tiles_x;
            t.tile_base[j] = (int)tiles;
            tiles += p.tiles;
        }
        t.njobs = n;
        hipLaunchKernelGGL(crf::gemm_jobs_kernel, dim3((unsigned)tiles), dim3(crf::GM_BLOCK), 0, st, t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" int crfconv_gemm_supported(int64_t M, int N, int K) {
    return (M >= 1 && M < (int64_t)1 << 31 && N >= 1 && K >= 1 && N < (1 << 24) && K < (1 << 24)) ? 1 : 0;
}

// C [M, N] = A [M, K] · B + bias + addend.  b_is_nk != 0: B is [N, K] row-major (the F.linear weight: C = A Bᵀ),
// else [K, N] row-major (C = A B: dX = gY · W with W [Co, Ci]).  bias [N] and addend [M, N] may be NULL; addend may alias C.
extern "C" int crfconv_gemm(const float* A, const float* B, const float* bias, const float* addend, int64_t M, int N, int K,
                            int b_is_nk, float* C, void* stream) {
    CRF_REQUIRE(A != nullptr && B != nullptr && C != nullptr, CRF_ERR_ARG, "null operand");
    CRF_REQUIRE(crfconv_gemm_supported(M, N, K), CRF_ERR_UNSUPPORTED, "gemm %lld x %d x %d: shape out of range", (long long)M, N, K);
    hipStream_t st = crf::as_stream(stream);
    // 16-byte accesses; odd widths (13-class logits) go element by element
    crf::gm_dispatch(M, N, b_is_nk != 0, N % 4 == 0 && K % 4 == 0, [&](auto form, dim3 grid) {
        using T = decltype(form);
        hipLaunchKernelGGL((crf::gemm_kernel<T::WM, T::WN, T::WR, T::WC, T::BNK, T::VEC>), grid, dim3(crf::GM_BLOCK), 0, st, A, B, bias, addend,
                           (int)M, N, K, C);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// The eval-mode MLP block as ONE launch on the tiled product: C = lrelu(add_rn(fmaf(a, A · B (+ bias), b), skip), slope) with
// coef = the BatchNorm's coefficient rows a | b ([>= 2][N]: crfconv_bn_eval_coef_jobs, crfconv_bn_forward); skip [M, N] may be NULL,
// slope 1 = no activation.  The tile shape crfconv_gemm picks for (M, N, K), the same summation order: bit-identical to that product
// followed by crfconv_bn_apply (and crfconv_add_lrelu with a skip).  N % 4 == 0.
extern "C" int crfconv_gemm_bn_act(const float* A, const float* B, const float* bias, const float* coef, const float* skip, float slope,
                                   int64_t M, int N, int K, int b_is_nk, float* C, void* stream) {
    CRF_REQUIRE(A != nullptr && B != nullptr && C != nullptr && coef != nullptr, CRF_ERR_ARG, "null operand");
    CRF_REQUIRE(crfconv_gemm_supported(M, N, K), CRF_ERR_UNSUPPORTED, "gemm %lld x %d x %d: shape out of range", (long long)M, N, K);
    CRF_REQUIRE(N % 4 == 0, CRF_ERR_UNSUPPORTED, "N=%d must be a multiple of 4", N);
    hipStream_t st = crf::as_stream(stream);
    crf::gm_dispatch(M, N, b_is_nk != 0, K % 4 == 0, [&](auto form, dim3 grid) {
        using T = decltype(form);
        hipLaunchKernelGGL((crf::gemm_bn_act_kernel<T::WM, T::WN, T::WR, T::WC, T::BNK, T::VEC>), grid, dim3(crf::GM_BLOCK), 0, st, A, B, bias, skip,
                           (int)M, N, K, C, coef, slope);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
