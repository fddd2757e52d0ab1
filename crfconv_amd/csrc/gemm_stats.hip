// The tiled product that leaves BatchNorm statistic records (the STATS form of gemm_tile.hpp): C [M, N] = A [M, K] B^T with one record
// per 16-row group and channel from the epilogue, so the statistics pass over C never runs -- the Linear of the coarse-level MLP blocks
// in training (models/common.py:30,35).  Up to 4 independent products per launch; with the UV operand, the PointConv combine of
// uv_fold.hpp formed on load.
#include "gemm_tile.hpp"

namespace crf {

struct GemmStatsJobs {                                  // (slots at or past njobs are never read)
    const float* A[GG_MAX]; const float* B[GG_MAX]; float* C[GG_MAX]; float* rec[GG_MAX];
    int M[GG_MAX], N[GG_MAX], K[GG_MAX], tiles_x[GG_MAX], wide[GG_MAX];
    int tile_base[GG_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(GM_BLOCK) void gemm_stats_jobs_kernel(const GemmStatsJobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.tile_base[j + 1] <= (int)blockIdx.x) ++j;
    const unsigned local = blockIdx.x - (unsigned)t.tile_base[j];
    const unsigned tx = (unsigned)uni(t.tiles_x[j]);
    const unsigned bx = (unsigned)uni((int)(local % tx)), by = (unsigned)uni((int)(local / tx));
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<1, 2, 2, 2, true, false>()];
    if (uni(t.wide[j]))
        gemm_tile<1, 2, 2, 2, true, true, false, true>(uni(t.A[j]), uni(t.B[j]), nullptr, nullptr, uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]), GemmPro(),
                                                       uni(t.rec[j]), bx, by, lds);
    else
        gemm_tile<1, 1, 2, 2, true, true, false, true>(uni(t.A[j]), uni(t.B[j]), nullptr, nullptr, uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]), GemmPro(),
                                                       uni(t.rec[j]), bx, by, lds);
}
// crfconv_gemm_stats (one job, the same tiles) with the UV operand
__global__ __launch_bounds__(GM_BLOCK) void gemm_stats_uv_kernel(const float* __restrict__ U, const float* __restrict__ B, const int M, const int N,
                                                                 const int K, float* __restrict__ C, float* __restrict__ rec, const int tiles_x,
                                                                 const int wide, const UvFold uv) {
    const unsigned tx = (unsigned)tiles_x;
    const unsigned bx = (unsigned)uni((int)(blockIdx.x % tx)), by = (unsigned)uni((int)(blockIdx.x / tx));
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<1, 2, 2, 2, true, false>()];
    __shared__ __attribute__((aligned(16))) float s_uv[2 * GM_UV_MAXK];
    if (wide)
        gemm_tile<1, 2, 2, 2, true, true, false, true, true>(U, B, nullptr, nullptr, M, N, K, C, GemmPro(), rec, bx, by, lds, 0, &uv, s_uv);
    else
        gemm_tile<1, 1, 2, 2, true, true, false, true, true>(U, B, nullptr, nullptr, M, N, K, C, GemmPro(), rec, bx, by, lds, 0, &uv, s_uv);
}

}  // namespace crf

extern "C" size_t crfconv_gemm_stat_records(int64_t M) { return M < 1 ? 0 : (size_t)(2 * ((M + 31) / 32)); }

// C [M, N] = A [M, K] B^T (B [N, K]: the F.linear weight) with BatchNorm statistic records of C from the epilogue: stat_rec
// float [crfconv_gemm_stat_records(M)][N][4] = {shift, rows, sum (v - shift), sum (v - shift)^2} per 16-row group and channel,
// to be combined by crfconv_bn_coef_from_records.  N, K multiples of 4.
extern "C" int crfconv_gemm_stats(const float* A, const float* B, int64_t M, int N, int K, float* C, float* stat_rec, void* stream) {
    crf_gemm_stats_job job;
    job.A = A; job.B = B; job.M = M; job.N = N; job.K = K; job.C = C; job.stat_rec = stat_rec;
    return crfconv_gemm_stats_jobs(&job, 1, stream);
}

// crfconv_gemm_stats for up to 4 independent products in ONE launch: C_j = A_j B_j^T with the statistic records of each C_j.
extern "C" int crfconv_gemm_stats_jobs(const crf_gemm_stats_job* jobs, int njobs, void* stream) {
    CRF_REQUIRE(jobs && njobs >= 1 && njobs <= crf::GG_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d)", crf::GG_MAX, njobs);
    crf::GemmStatsJobs t{};
    int64_t tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const crf_gemm_stats_job& b = jobs[j];
        CRF_REQUIRE(b.A && b.B && b.C && b.stat_rec, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(b.M >= 1 && b.M < ((int64_t)1 << 31) && b.N >= 4 && b.K >= 4 && b.N % 4 == 0 && b.K % 4 == 0, CRF_ERR_UNSUPPORTED,
                    "job %d: gemm_stats %lld x %d x %d: N and K must be multiples of 4", j, (long long)b.M, b.N, b.K);
        crf::GmTilePlan p;
        if (int rc = crf::gm_tile_plan(b.M, b.N, true, tiles, p)) return rc;
        t.A[j] = b.A; t.B[j] = b.B; t.C[j] = b.C; t.rec[j] = b.stat_rec; t.M[j] = (int)b.M; t.N[j] = b.N; t.K[j] = b.K;
        t.tiles_x[j] = p.tiles_x; t.wide[j] = p.wide;
        t.tile_base[j] = (int)tiles;
        tiles += p.tiles;
    }
    t.njobs = njobs;
    hipLaunchKernelGGL(crf::gemm_stats_jobs_kernel, dim3((unsigned)tiles), dim3(crf::GM_BLOCK), 0, crf::as_stream(stream), t);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// crfconv_pointconv_combine(f) + crfconv_gemm_stats(f->out, B) in one launch: the A operand out = a2 U + (a2 shift + b2) V is formed while
// its chunks are staged and stored to f->out by the first column tiles (K <= 128 input channels).
extern "C" int crfconv_gemm_stats_uv_supported(int64_t M, int N, int K) {
    return (M >= 1 && M < ((int64_t)1 << 31) && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0 && K <= crf::GM_UV_MAXK) ? 1 : 0;
}
extern "C" int crfconv_gemm_stats_uv(const crf_uv_fold* f, const float* B, int64_t M, int N, int K, float* C, float* stat_rec, void* stream) {
    CRF_REQUIRE(B && C && stat_rec, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(crf::uv_fold_complete(f), CRF_ERR_ARG, "combine record: null pointer, or running statistics not as a pair");
    CRF_REQUIRE(crfconv_gemm_stats_uv_supported(M, N, K), CRF_ERR_UNSUPPORTED, "gemm_stats_uv %lld x %d x %d: N, K multiples of 4, K <= %d",
                (long long)M, N, K, crf::GM_UV_MAXK);
    const crf::UvFold uv = crf::uv_fold_args(f);
    crf::GmTilePlan p;
    if (int rc = crf::gm_tile_plan(M, N, true, 0, p)) return rc;
    hipLaunchKernelGGL(crf::gemm_stats_uv_kernel, dim3((unsigned)p.tiles), dim3(crf::GM_BLOCK), 0, crf::as_stream(stream), f->U, B, (int)M, N, K, C,
                       stat_rec, p.tiles_x, p.wide, uv);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
