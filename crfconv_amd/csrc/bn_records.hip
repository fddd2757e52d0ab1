// BatchNorm from the per-workgroup statistic records that the Linear kernels leave in their epilogue (linear_fwd.hpp, gemm_stats.hip)
// instead of a statistics pass over y: the coefficients alone (bn_finalize_records_kernel), or coefficients and apply
// (+ the ResNet join) in one launch, for one layer or up to four independent ones.
#include "common.hpp"

namespace crf {

// Combine the per-block {shift, n, sum, sumsq} records into BatchNorm coefficients (Chan's parallel variance in
// float64), same outputs as bn_finalize_kernel.  rec [nrec][C][4]: a thread reads whole 16-byte tuples, 16 adjacent
// channels per record-lane (256 contiguous bytes), 64 record-lanes per workgroup; record-lanes fold by shuffles
// inside a wavefront and through LDS across the 16 wavefronts, always in the same order.
constexpr int FR_BLOCK = 1024, FR_CH = 16, FR_RL = FR_BLOCK / FR_CH;
// (device body: `slab` = which 16 channels; write != 0: this caller publishes coef / running statistics.  Threads < FR_CH of a valid
// channel return with ab = {a, b}; every other thread returns false.)
template <int FR_UN = 8>      // tuples of a thread in flight at once (nrec <= 1024: two round trips instead of four dependent ones; the
                               // order a thread visits its tuples in -- hence every sum -- does not depend on it)
__device__ __forceinline__ bool bn_finalize_records_body(const float* __restrict__ rec, int nrec, int64_t M, int C,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float* __restrict__ run_mean, float* __restrict__ run_var, float momentum,
                                                         float* __restrict__ coef, int slab, bool write, float (&ab)[2]) {
    __shared__ double s_red[FR_BLOCK / WAVE][2][FR_CH];
    const int cl = threadIdx.x & (FR_CH - 1), rl = threadIdx.x >> 4;
    const int c = slab * FR_CH + cl;
    const bool cv = c < C;
    const int cc = cv ? c : C - 1;
    // every record is re-based on the shift of record 0 (a sample value, so |shift - mean| ~ sigma: no cancellation
    // problem in float64)
    const double s0 = rec[(int64_t)cc * 4];
    double S1 = 0.0, S2 = 0.0;
    for (int r0 = rl; r0 < nrec; r0 += FR_UN * FR_RL) {
        float4 v[FR_UN];
#pragma unroll
        for (int u = 0; u < FR_UN; ++u) {
            const int r = r0 + u * FR_RL;
            v[u] = r < nrec ? *reinterpret_cast<const float4*>(rec + ((int64_t)r * C + cc) * 4)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < FR_UN; ++u) {
            const double nb = v[u].y;
            if (nb > 0.0) {
                const double d = (double)v[u].x - s0, a = v[u].z, b = v[u].w;
                S1 += a + nb * d;
                S2 += b + 2.0 * d * a + nb * d * d;
            }
        }
    }
    // lanes l, l ^ 16, l ^ 32, l ^ 48 of a wavefront hold the same channel
    S1 += __shfl_xor(S1, 16, WAVE); S2 += __shfl_xor(S2, 16, WAVE);
    S1 += __shfl_xor(S1, 32, WAVE); S2 += __shfl_xor(S2, 32, WAVE);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < FR_CH) { s_red[wave][0][cl] = S1; s_red[wave][1][cl] = S2; }
    __syncthreads();
    if (threadIdx.x >= FR_CH || !cv) return false;
    S1 = 0.0; S2 = 0.0;
    for (int w = 0; w < FR_BLOCK / WAVE; ++w) { S1 += s_red[w][0][cl]; S2 += s_red[w][1][cl]; }
    const double m1 = S1 / (double)M;
    const double mean = s0 + m1;
    const double m2 = S2 - S1 * m1;
    double var = m2 / (double)M;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[c] * rstd;
    ab[0] = (float)a;
    ab[1] = (float)((double)beta[c] - a * mean);
    if (!write) return true;
    coef[c] = ab[0];
    coef[C + c] = ab[1];
    coef[2 * C + c] = (float)mean;
    coef[3 * C + c] = (float)rstd;
    if (run_mean != nullptr) {
        const double unb = M > 1 ? var * ((double)M / (double)(M - 1)) : var;
        run_mean[c] = (float)((1.0 - (double)momentum) * (double)run_mean[c] + (double)momentum * mean);
        run_var[c] = (float)((1.0 - (double)momentum) * (double)run_var[c] + (double)momentum * unb);
    }
    return true;
}
__global__ __launch_bounds__(FR_BLOCK) void bn_finalize_records_kernel(const float* __restrict__ rec, int nrec, int64_t M,
                                                                       int C, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, float eps,
                                                                       float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                       float momentum, float* __restrict__ coef) {
    float ab[2];
    bn_finalize_records_body(rec, nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef, blockIdx.x, true, ab);
}

// Coefficients AND apply in one launch (crfconv_bn_apply_from_records): a workgroup = one 16-channel slab x one row tile; it combines
// the records of ITS slab exactly as bn_finalize_records_kernel does (same threads, same order: identical coefficients; the
// workgroups of row tile 0 publish them and update the running statistics), then streams y = lrelu(a x + b) over its rows -- 64-byte
// row pieces, four lanes per row.  The 512-record combine is redundant per row tile (131 KB of L2 reads per workgroup) and buys the
// ~6 us coefficient launch that used to sit between every Linear and its BatchNorm apply pass.
template <bool ADD, int UN = 8>      // ADD: y = lrelu(a x + b + skip, slope) -- the ResNet join (crfconv_bn_apply_add's arithmetic)
__device__ __forceinline__ void bn_apply_records_body(const float* __restrict__ rec, int nrec, int64_t M, int C,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float eps, float* __restrict__ run_mean, float* __restrict__ run_var,
                                                      float momentum, float* __restrict__ coef, const float* __restrict__ x,
                                                      const float* __restrict__ skip, float slope, int rows_per_tile,
                                                      float* __restrict__ y, const int slab, const int tile) {
    __shared__ float s_ab[2][FR_CH];
    float ab[2];
    // grid = (row tiles, slabs): the workgroups that read the two / four 64-byte pieces of the same 128-byte lines are `tiles` apart in
    // dispatch order, and tiles is a multiple of 8 -- they land on the same XCD, whose L2 then fetches each line from HBM once
    const int q = threadIdx.x & 3, rl = threadIdx.x >> 2;            // 4 channel quads x 256 rows per pass
    const int c = slab * FR_CH + 4 * q;
    const bool cok = c < C;
    const int64_t r0 = (int64_t)tile * rows_per_tile;
    const int64_t r1 = r0 + rows_per_tile < M ? r0 + rows_per_tile : M;
    // the rows of the FIRST pass (the only one at <= 1024 rows per tile) are requested before the records are combined: their round
    // trip runs beside the combine's two instead of behind them
    float4 v[4];
    [[maybe_unused]] float4 k[ADD ? 4 : 1];
    auto request = [&](int64_t rb) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = rb + (int64_t)u * (FR_BLOCK / 4);
            const bool in = cok && r < r1;
            v[u] = in ? *reinterpret_cast<const float4*>(x + r * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (ADD) k[u] = in ? *reinterpret_cast<const float4*>(skip + r * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
#ifndef BN_APPLY_PREFETCH_
#define BN_APPLY_PREFETCH_ 1
#endif
    if (BN_APPLY_PREFETCH_) request(r0 + rl);
    if (bn_finalize_records_body<UN>(rec, nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef, slab, tile == 0, ab)) {
        s_ab[0][threadIdx.x] = ab[0];
        s_ab[1][threadIdx.x] = ab[1];
    }
    __syncthreads();
    if (!cok) return;
    const float4 a = *reinterpret_cast<const float4*>(&s_ab[0][4 * q]), b = *reinterpret_cast<const float4*>(&s_ab[1][4 * q]);
    for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (FR_BLOCK / 4)) {
        if (!BN_APPLY_PREFETCH_ || rb != r0 + rl) request(rb);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = rb + (int64_t)u * (FR_BLOCK / 4);
            if (r >= r1) continue;
            float4 o = make_float4(fmaf(a.x, v[u].x, b.x), fmaf(a.y, v[u].y, b.y), fmaf(a.z, v[u].z, b.z), fmaf(a.w, v[u].w, b.w));
            if constexpr (ADD) {
                o.x = add_rn(o.x, k[u].x); o.y = add_rn(o.y, k[u].y); o.z = add_rn(o.z, k[u].z); o.w = add_rn(o.w, k[u].w);
            }
            o.x = o.x > 0.f ? o.x : slope * o.x;
            o.y = o.y > 0.f ? o.y : slope * o.y;
            o.z = o.z > 0.f ? o.z : slope * o.z;
            o.w = o.w > 0.f ? o.w : slope * o.w;
            *reinterpret_cast<float4*>(y + r * C + c) = o;
        }
    }
}

template <bool ADD>
__global__ __launch_bounds__(FR_BLOCK) void bn_apply_records_kernel(const float* __restrict__ rec, int nrec, int64_t M, int C,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float eps, float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                    float momentum, float* __restrict__ coef, const float* __restrict__ x,
                                                                    const float* __restrict__ skip, float slope, int rows_per_tile,
                                                                    float* __restrict__ y) {
    bn_apply_records_body<ADD>(rec, nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef, x, skip, slope, rows_per_tile, y,
                               blockIdx.y, blockIdx.x);
}
// The same for up to 4 independent layers in one launch (crfconv_bn_apply_from_records_jobs): the workgroups of the jobs laid end to end.
constexpr int BA_MAX = 4;
struct BnApplyJobs {
    const float* rec[BA_MAX]; const float* gamma[BA_MAX]; const float* beta[BA_MAX]; float* run_mean[BA_MAX]; float* run_var[BA_MAX];
    float* coef[BA_MAX]; const float* x[BA_MAX]; const float* skip[BA_MAX]; float* y[BA_MAX];
    long long M[BA_MAX];
    int nrec[BA_MAX], C[BA_MAX], rows_per_tile[BA_MAX], tiles[BA_MAX];
    float eps[BA_MAX], momentum[BA_MAX], slope[BA_MAX];
    int blk_base[BA_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(FR_BLOCK) void bn_apply_records_jobs_kernel(const BnApplyJobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blockIdx.x) ++j;
    const int local = (int)blockIdx.x - t.blk_base[j];
    const int tiles = uni(t.tiles[j]);
    const int tile = uni(local % tiles), slab = uni(local / tiles);
    const float* rec = uni(t.rec[j]); const float* gamma = uni(t.gamma[j]); const float* beta = uni(t.beta[j]);
    float* run_mean = uni(t.run_mean[j]); float* run_var = uni(t.run_var[j]); float* coef = uni(t.coef[j]);
    const float* x = uni(t.x[j]); const float* skip = uni(t.skip[j]); float* y = uni(t.y[j]);
    const long long M = uni(t.M[j]);
    const int nrec = uni(t.nrec[j]), C = uni(t.C[j]), rows = uni(t.rows_per_tile[j]);
    const float eps = uni(t.eps[j]), momentum = uni(t.momentum[j]), slope = uni(t.slope[j]);
    if (skip != nullptr) bn_apply_records_body<true, 4>(rec, nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef, x, skip, slope, rows, y, slab, tile);
    else bn_apply_records_body<false, 4>(rec, nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef, x, nullptr, slope, rows, y, slab, tile);
}

}  // namespace crf

// BatchNorm coefficients from the records written by crfconv_linear_forward (instead of a statistics pass).
extern "C" int crfconv_bn_coef_from_records(const float* stat_rec, int64_t M, int C, const float* gamma,
                                            const float* beta, float* run_mean, float* run_var, float momentum,
                                            float eps, float* coef, crf_stream_t stream) {
    CRF_REQUIRE(stat_rec && gamma && beta && coef, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0 && C > 0, CRF_ERR_ARG, "bad shape");
    return crfconv_bn_coef_from_nrecords(stat_rec, (int64_t)crfconv_linear_forward_stat_records(M), M, C, gamma, beta, run_mean, run_var,
                                         momentum, eps, coef, stream);
}

// The same with an explicit record count (records of crfconv_gemm_stats: one per 16-row group).
extern "C" int crfconv_bn_coef_from_nrecords(const float* stat_rec, int64_t nrec, int64_t M, int C, const float* gamma,
                                             const float* beta, float* run_mean, float* run_var, float momentum,
                                             float eps, float* coef, crf_stream_t stream) {
    CRF_REQUIRE(stat_rec && gamma && beta && coef, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0 && C > 0 && nrec > 0 && nrec < ((int64_t)1 << 31), CRF_ERR_ARG, "bad shape");
    hipLaunchKernelGGL(crf::bn_finalize_records_kernel, dim3((C + crf::FR_CH - 1) / crf::FR_CH), dim3(crf::FR_BLOCK), 0, crf::as_stream(stream), stat_rec,
                       (int)nrec, M, C, gamma, beta, eps, run_mean, run_var, momentum, coef);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// crfconv_bn_coef_from_records followed by crfconv_bn_apply (skip == NULL) or crfconv_bn_apply_add (the ResNet join) in ONE launch:
// identical coef / running statistics / y.  C % 4 == 0.
// row tiles of one apply launch: ~`wgs` workgroups in all -- one per CU: 116-128 registers x 1024 threads is one workgroup per CU, and
// every workgroup pays the records' combine (step, one box: 128 workgroups 4.163 ms, 192 4.136, 256 4.136, 320 4.159, 512 4.153); a
// row tile is a multiple of the 1024 rows one pass covers
#ifndef BN_APPLY_WGS_
#define BN_APPLY_WGS_ 256
#endif
static void bn_apply_plan(int64_t M, int C, int wgs, int64_t& tiles, int64_t& rows) {
    const int slabs = (C + crf::FR_CH - 1) / crf::FR_CH;
    tiles = wgs / slabs;
    if (tiles < 1) tiles = 1;
    rows = (M + tiles - 1) / tiles;
    rows = (rows + 1023) / 1024 * 1024;
    tiles = (M + rows - 1) / rows;
    if (tiles > 8) tiles = (tiles + 7) / 8 * 8;          // (tiles past the end of the rows have nothing to apply; see the kernel for the 8)
}

extern "C" int crfconv_bn_apply_from_records(const float* stat_rec, int64_t nrec, const float* x, int64_t M, int C, const float* gamma,
                                             const float* beta, float* run_mean, float* run_var, float momentum, float eps,
                                             const float* skip, float slope, float* coef, float* y, crf_stream_t stream) {
    CRF_REQUIRE(stat_rec && x && gamma && beta && coef && y, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0 && C >= 4 && C % 4 == 0 && nrec > 0 && nrec < ((int64_t)1 << 31), CRF_ERR_ARG, "bad shape");
    const int slabs = (C + crf::FR_CH - 1) / crf::FR_CH;
    int64_t tiles, rows;
    bn_apply_plan(M, C, BN_APPLY_WGS_, tiles, rows);
    const dim3 grid((unsigned)tiles, (unsigned)slabs), blk(crf::FR_BLOCK);
    if (skip != nullptr)
        hipLaunchKernelGGL(crf::bn_apply_records_kernel<true>, grid, blk, 0, crf::as_stream(stream), stat_rec, (int)nrec, M, C, gamma, beta, eps,
                           run_mean, run_var, momentum, coef, x, skip, slope, (int)rows, y);
    else
        hipLaunchKernelGGL(crf::bn_apply_records_kernel<false>, grid, blk, 0, crf::as_stream(stream), stat_rec, (int)nrec, M, C, gamma, beta, eps,
                           run_mean, run_var, momentum, coef, x, skip, slope, (int)rows, y);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_bn_apply_from_records_jobs(const crf_bn_apply_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs && njobs >= 1 && njobs <= crf::BA_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d)", crf::BA_MAX, njobs);
    crf::BnApplyJobs t;
    int64_t blocks = 0;
    for (int j = 0; j <= crf::BA_MAX; ++j) {
        t.blk_base[j] = (int)blocks;
        if (j >= crf::BA_MAX) break;
        if (j >= njobs) {
            t.rec[j] = nullptr; t.gamma[j] = nullptr; t.beta[j] = nullptr; t.run_mean[j] = nullptr; t.run_var[j] = nullptr; t.coef[j] = nullptr;
            t.x[j] = nullptr; t.skip[j] = nullptr; t.y[j] = nullptr; t.M[j] = 0; t.nrec[j] = 0; t.C[j] = 4; t.rows_per_tile[j] = 1024; t.tiles[j] = 1;
            t.eps[j] = 0.f; t.momentum[j] = 0.f; t.slope[j] = 1.f;
            continue;
        }
        const crf_bn_apply_job& b = jobs[j];
        CRF_REQUIRE(b.stat_rec && b.x && b.gamma && b.beta && b.coef && b.y, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(b.M > 0 && b.C >= 4 && b.C % 4 == 0 && b.nrec > 0 && b.nrec < ((int64_t)1 << 31), CRF_ERR_ARG, "job %d: bad shape", j);
        int64_t tiles, rows;
        bn_apply_plan(b.M, b.C, BN_APPLY_WGS_ / njobs, tiles, rows);
        t.rec[j] = b.stat_rec; t.gamma[j] = b.gamma; t.beta[j] = b.beta; t.run_mean[j] = b.run_mean; t.run_var[j] = b.run_var; t.coef[j] = b.coef;
        t.x[j] = b.x; t.skip[j] = b.skip; t.y[j] = b.y; t.M[j] = (long long)b.M; t.nrec[j] = (int)b.nrec; t.C[j] = b.C; t.rows_per_tile[j] = (int)rows;
        t.tiles[j] = (int)tiles; t.eps[j] = b.eps; t.momentum[j] = b.momentum; t.slope[j] = b.slope;
        blocks += tiles * ((b.C + crf::FR_CH - 1) / crf::FR_CH);
        CRF_REQUIRE(blocks < ((int64_t)1 << 31), CRF_ERR_UNSUPPORTED, "too many workgroups in one batch");
    }
    t.njobs = njobs;
    hipLaunchKernelGGL(crf::bn_apply_records_jobs_kernel, dim3((unsigned)blocks), dim3(crf::FR_BLOCK), 0, crf::as_stream(stream), t);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
