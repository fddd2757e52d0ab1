// Weight gradient of the per-point Linear layers:  dW[co, ci] = sum_m G[m, co] * X[m, ci]
// (+ optional bias gradient db[co] = sum_m G[m, co]).
//
// These are the path's genuinely dense contractions (models/common.py:30,35 -- every MLP.lin), but
// with a reduction dimension of m = 10^4..10^5 rows and a tiny [Co, Ci] output, which is exactly
// the shape vendor GEMMs handle worst (rocBLAS: 140-420 us at m = 163840; streaming the operands once
// takes 5-20 us).  Here each wavefront streams its slice of rows straight from HBM into fp32 MFMA
// (v_mfma_f32_16x16x4_f32: exact f32, fmaf-chain numerics): lane l of a k-step holds
//   A[i = l & 15][k = l >> 4] = G[row0 + (l >> 4)][co0 + (l & 15)]
//   B[k = l >> 4][j = l & 15] = X[row0 + (l >> 4)][ci0 + (l & 15)]
// i.e. the row-major operands ARE the fragment layout -- no transpose, no LDS staging.  Accumulator
// tiles stay in registers for the whole slice; waves of a block combine through LDS; block partials
// are summed in a fixed order by a second kernel (bitwise reproducible, no float atomics).  That second kernel and its batched
// end-of-pass forms (reduce_jobs_kernel; reduce_both_kernel, which also takes the float64 sums of reduce64_body.hpp) live here too.
#include "common.hpp"
#include "wgrad_body.hpp"
#include "reduce64_body.hpp"

namespace crf {

template <int TCO, int TCI>
__global__ __launch_bounds__(WG_BLOCK) void wgrad_kernel(const float* __restrict__ G,
                                                         const float* __restrict__ X, int64_t M, int Co,
                                                         int Ci, int rows_per_block,
                                                         float* __restrict__ partial /*[nblk][Co][Ci]*/,
                                                         float* __restrict__ partial_b /*[nblk][Co] or null*/) {
    __shared__ float s_red[WG_RED_BUFS * TCO * TCI * 256];
    __shared__ float s_b[WG_WAVES * TCO * 16];
    wgrad_body<TCO, TCI>(G, X, M, Co, Ci, rows_per_block, partial, partial_b, blockIdx.x, blockIdx.y, blockIdx.z, s_red, s_b);
}

// Every tile class in ONE launch (round 4): the jobs of the small classes -- five launches of 40-240 workgroups, 7-12 us each, behind
// the <4, 4> launch of the step -- run beside the large ones.  The workgroup looks its job up as above and dispatches on the job's
// class; one LDS buffer of the largest class (32 KB: wgrad_body's two-round sum), the register budget of the largest (the small classes' jobs are few).
__global__ __launch_bounds__(WG_BLOCK) void wgrad_jobs_any_kernel(const WgJobTable t) {
    __shared__ float s_red[WG_RED_BUFS * 4 * 4 * 256];
    __shared__ float s_b[WG_WAVES * 4 * 16];
    wgrad_any_run(t, (int)blockIdx.x, s_red, s_b);
}

// out[slot] = sum_b partial[b][slot] for 64 consecutive slots per workgroup: lanes run along the slots (256-byte
// coalesced rows of the partial slabs), the 4 wavefronts take b = w, w + 4, ... with four loads in flight each, and
// combine through LDS in the fixed order w = 0..3 -- bitwise reproducible, and identical between the single and the
// batched entry point.
__device__ __forceinline__ void reduce_slab64(const float* __restrict__ partial, int nblk, int nslots, int slot0,
                                              float* __restrict__ out, float (*s_part)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int slot = slot0 + lane;
    const bool ok = slot < nslots;
    const float* p = partial + (ok ? slot : 0);
    // eight slabs in flight per wavefront: the reduction is a chain of dependent L2 / HBM round trips, not bandwidth
    // (512 slabs of an 8 x 8 gradient took 10.5 us with four in flight)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int b = w;
    for (; b + 28 < nblk; b += 32) {
        const float v0 = p[(int64_t)b * nslots], v1 = p[(int64_t)(b + 4) * nslots], v2 = p[(int64_t)(b + 8) * nslots];
        const float v3 = p[(int64_t)(b + 12) * nslots], v4 = p[(int64_t)(b + 16) * nslots], v5 = p[(int64_t)(b + 20) * nslots];
        const float v6 = p[(int64_t)(b + 24) * nslots], v7 = p[(int64_t)(b + 28) * nslots];
        a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        a0 += v4; a1 += v5; a2 += v6; a3 += v7;
    }
    for (; b + 12 < nblk; b += 16) {
        a0 += p[(int64_t)b * nslots];
        a1 += p[(int64_t)(b + 4) * nslots];
        a2 += p[(int64_t)(b + 8) * nslots];
        a3 += p[(int64_t)(b + 12) * nslots];
    }
    for (; b < nblk; b += 4) a0 += p[(int64_t)b * nslots];
    s_part[w][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (w == 0 && ok) out[slot] = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int nblk,
                                                           int nslots, float* __restrict__ out) {
    __shared__ float s_part[4][64];
    reduce_slab64(partial, nblk, nslots, blockIdx.x * 64, out, s_part);
}

// Many reductions in one launch: job j sums nblk[j] partial slabs of nslots[j] floats into out[j].  The table travels
// in the kernel arguments (no device copy, capturable into a hipGraph); workgroup g serves one 64-slot group of one
// job (group_begin = prefix sum of ceil(nslots / 64)).
constexpr int RJ_MAX = 96;
struct ReduceJobTable {
    const float* partial[RJ_MAX];
    float* out[RJ_MAX];
    int nblk[RJ_MAX];
    int nslots[RJ_MAX];
    int group_begin[RJ_MAX + 1];
    int njobs;
};

__global__ __launch_bounds__(256) void reduce_jobs_kernel(const ReduceJobTable tbl) {
    __shared__ float s_part[4][64];
    const int g = blockIdx.x;
    int lo = 0, hi = tbl.njobs;                       // largest j with group_begin[j] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tbl.group_begin[mid] <= g) lo = mid; else hi = mid;
    }
    reduce_slab64(tbl.partial[lo], tbl.nblk[lo], tbl.nslots[lo], (g - tbl.group_begin[lo]) * 64, tbl.out[lo], s_part);
}


// crfconv_reduce_jobs AND crfconv_reduce_jobs_f64 in one launch (the end of a backward pass runs both, on independent inputs: the
// float64 sums are ~650 wavefront-per-slot workgroups of latency, the float ones ~12 000 workgroups of bandwidth): the first n64
// workgroups take the float64 table -- they start first --, the others the float one.
__global__ __launch_bounds__(256) void reduce_both_kernel(const ReduceJobTable tbl, const Reduce64Table t64, const int n64) {
    __shared__ float s_part[4][64];
    if ((int)blockIdx.x < n64) {
        reduce_jobs_f64_body(t64, blockIdx.x);
        return;
    }
    const int g = (int)blockIdx.x - n64;
    int lo = 0, hi = tbl.njobs;                       // largest j with group_begin[j] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tbl.group_begin[mid] <= g) lo = mid; else hi = mid;
    }
    reduce_slab64(tbl.partial[lo], tbl.nblk[lo], tbl.nslots[lo], (g - tbl.group_begin[lo]) * 64, tbl.out[lo], s_part);
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_linear_wgrad_workspace(int64_t M, int Co, int Ci) {
    if (M <= 0 || Co <= 0 || Ci <= 0) return 0;
    const WgPlan p = wg_plan(M, Co, Ci);
    return sizeof(float) * (size_t)p.nblk * ((size_t)Co * Ci + (size_t)Co) + 256;
}

static int wgrad_launch(const float* G, const float* X, int64_t M, int Co, int Ci, const WgPlan& p, float* partial,
                        float* partial_b, hipStream_t st) {
    const dim3 grid((unsigned)p.nblk, (unsigned)p.gy, (unsigned)p.gz), blk(WG_BLOCK);
#define WG(TA, TB) hipLaunchKernelGGL((wgrad_kernel<TA, TB>), grid, blk, 0, st, G, X, M, Co, Ci, p.rows_per_block, partial, partial_b)
    switch (p.tco * 10 + p.tci) {
        case 11: WG(1, 1); break;
        case 12: WG(1, 2); break;
        case 14: WG(1, 4); break;
        case 21: WG(2, 1); break;
        case 22: WG(2, 2); break;
        case 24: WG(2, 4); break;
        case 41: WG(4, 1); break;
        case 42: WG(4, 2); break;
        default: WG(4, 4); break;
    }
#undef WG
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_linear_wgrad_partial(const float* G, const float* X, int64_t M, int Co, int Ci, int want_bias,
                                            void* workspace, size_t workspace_bytes, int* nblk_out, crf_stream_t stream) {
    CRF_REQUIRE(G && X && workspace && nblk_out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0 && Co > 0 && Ci > 0 && Co <= 4096 && Ci <= 4096, CRF_ERR_ARG, "bad shape M=%lld Co=%d Ci=%d",
                (long long)M, Co, Ci);
    CRF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, CRF_ERR_ARG, "workspace must be 256-byte aligned");
    CRF_REQUIRE(workspace_bytes >= crfconv_linear_wgrad_workspace(M, Co, Ci), CRF_ERR_WORKSPACE, "workspace too small");
    const WgPlan p = wg_plan(M, Co, Ci);
    float* partial = reinterpret_cast<float*>(workspace);
    float* partial_b = want_bias ? partial + (size_t)p.nblk * Co * Ci : nullptr;
    *nblk_out = p.nblk;
    return wgrad_launch(G, X, M, Co, Ci, p, partial, partial_b, as_stream(stream));
}

extern "C" int crfconv_linear_wgrad_nblk(int64_t M, int Co, int Ci) {
    if (M <= 0 || Co <= 0 || Ci <= 0) return 0;
    return wg_plan(M, Co, Ci).nblk;
}

// crfconv_linear_wgrad_partial for several layers at once (jobs: host array): one launch per tile class present among the jobs
// (at most nine, typically one or two) instead of one per layer; identical partial slabs.
extern "C" int crfconv_linear_wgrad_partial_jobs(const crf_wgrad_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j = 0; j < njobs; ++j) {
        const crf_wgrad_job& jb = jobs[j];
        CRF_REQUIRE(jb.G && jb.X && jb.workspace, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(jb.M > 0 && jb.M < ((int64_t)1 << 31) && jb.Co > 0 && jb.Ci > 0 && jb.Co <= 4096 && jb.Ci <= 4096, CRF_ERR_ARG,
                    "job %d: bad shape M=%lld Co=%d Ci=%d", j, (long long)jb.M, jb.Co, jb.Ci);
        CRF_REQUIRE((reinterpret_cast<uintptr_t>(jb.workspace) & 255) == 0, CRF_ERR_ARG, "job %d: workspace must be 256-byte aligned", j);
        CRF_REQUIRE(jb.workspace_bytes >= crfconv_linear_wgrad_workspace(jb.M, jb.Co, jb.Ci), CRF_ERR_WORKSPACE, "job %d: workspace too small", j);
    }
    // jobs in the caller's order (longest first), WJ_MAX per launch
    for (int j0 = 0; j0 < njobs; j0 += WJ_MAX) {
        WgJobTable t;
        int64_t blocks = 0;
        const int n = njobs - j0 < WJ_MAX ? njobs - j0 : WJ_MAX;
        wg_fill_table(jobs + j0, n, t, blocks);
        CRF_REQUIRE(blocks < ((int64_t)1 << 31), CRF_ERR_UNSUPPORTED, "too many workgroups in one batch");
        hipLaunchKernelGGL(wgrad_jobs_any_kernel, dim3((unsigned)blocks), dim3(WG_BLOCK), 0, st, t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" int crfconv_reduce_jobs(const crf_reduce_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j0 = 0; j0 < njobs; j0 += RJ_MAX) {
        ReduceJobTable tbl;
        const int n = njobs - j0 < RJ_MAX ? njobs - j0 : RJ_MAX;
        int64_t total = 0;
        for (int j = 0; j < n; ++j) {
            const crf_reduce_job& jb = jobs[j0 + j];
            CRF_REQUIRE(jb.partial && jb.out && jb.nblk > 0 && jb.nslots > 0, CRF_ERR_ARG, "job %d is malformed", j0 + j);
            tbl.partial[j] = jb.partial;
            tbl.out[j] = jb.out;
            tbl.nblk[j] = jb.nblk;
            tbl.nslots[j] = jb.nslots;
            tbl.group_begin[j] = (int)total;
            total += (jb.nslots + 63) / 64;
            CRF_REQUIRE(total < ((int64_t)1 << 30), CRF_ERR_ARG, "too many slots in one batch");
        }
        for (int j = n; j <= RJ_MAX; ++j) tbl.group_begin[j] = (int)total;
        for (int j = n; j < RJ_MAX; ++j) { tbl.partial[j] = nullptr; tbl.out[j] = nullptr; tbl.nblk[j] = 0; tbl.nslots[j] = 0; }
        tbl.njobs = n;
        hipLaunchKernelGGL(reduce_jobs_kernel, dim3((unsigned)total), dim3(256), 0, st, tbl);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

// crfconv_reduce_jobs_f64 lives in pointconv_fold.hip; the header declares it.
// Both kinds of sums of a backward pass in ONE launch when each fits one table (96 float jobs, 32 float64 jobs): same results as the
// two calls.  Larger batches: the two calls.
extern "C" int crfconv_reduce_jobs_both(const crf_reduce_job* jobs, int njobs, const crf_reduce64_job* jobs64, int njobs64,
                                        crf_stream_t stream) {
    CRF_REQUIRE((jobs || njobs == 0) && (jobs64 || njobs64 == 0) && njobs >= 0 && njobs64 >= 0, CRF_ERR_ARG, "null pointer or negative count");
    if (njobs == 0 || njobs64 == 0 || njobs > RJ_MAX || njobs64 > R64_MAX) {
        if (njobs64 > 0)
            if (int rc = crfconv_reduce_jobs_f64(jobs64, njobs64, stream)) return rc;
        return njobs > 0 ? crfconv_reduce_jobs(jobs, njobs, stream) : CRF_OK;
    }
    ReduceJobTable tbl;
    int64_t total = 0;
    for (int j = 0; j < njobs; ++j) {
        const crf_reduce_job& jb = jobs[j];
        CRF_REQUIRE(jb.partial && jb.out && jb.nblk > 0 && jb.nslots > 0, CRF_ERR_ARG, "job %d is malformed", j);
        tbl.partial[j] = jb.partial; tbl.out[j] = jb.out; tbl.nblk[j] = jb.nblk; tbl.nslots[j] = jb.nslots;
        tbl.group_begin[j] = (int)total;
        total += (jb.nslots + 63) / 64;
    }
    for (int j = njobs; j <= RJ_MAX; ++j) tbl.group_begin[j] = (int)total;
    for (int j = njobs; j < RJ_MAX; ++j) { tbl.partial[j] = nullptr; tbl.out[j] = nullptr; tbl.nblk[j] = 0; tbl.nslots[j] = 0; }
    tbl.njobs = njobs;
    Reduce64Table t;
    int64_t waves = 0;
    for (int j = 0; j <= R64_MAX; ++j) {
        t.wave_base[j] = (int)waves;
        if (j < njobs64) {
            const crf_reduce64_job& jb = jobs64[j];
            CRF_REQUIRE(jb.partial && jb.out && jb.nblk > 0 && jb.nblk < ((int64_t)1 << 31) && jb.nslots > 0, CRF_ERR_ARG, "float64 job %d is malformed", j);
            t.partial[j] = jb.partial; t.out[j] = jb.out; t.is_float[j] = jb.is_float; t.nblk[j] = (int)jb.nblk; t.nslots[j] = jb.nslots;
            waves += jb.nslots;
        } else if (j < R64_MAX) {
            t.partial[j] = nullptr; t.out[j] = nullptr; t.is_float[j] = 0; t.nblk[j] = 0; t.nslots[j] = 0;
        }
    }
    t.njobs = njobs64;
    const int64_t n64 = cdiv(waves, 256 / WAVE);
    CRF_REQUIRE(total + n64 < ((int64_t)1 << 30), CRF_ERR_UNSUPPORTED, "too many slots in one batch");
    hipLaunchKernelGGL(reduce_both_kernel, dim3((unsigned)(total + n64)), dim3(256), 0, as_stream(stream), tbl, t, (int)n64);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_linear_wgrad(const float* G, const float* X, int64_t M, int Co, int Ci, float* dW,
                                    float* db, void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(G && X && dW && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0 && Co > 0 && Ci > 0 && Co <= 4096 && Ci <= 4096, CRF_ERR_ARG, "bad shape M=%lld Co=%d Ci=%d",
                (long long)M, Co, Ci);
    CRF_REQUIRE(workspace_bytes >= crfconv_linear_wgrad_workspace(M, Co, Ci), CRF_ERR_WORKSPACE, "workspace too small");
    const WgPlan p = wg_plan(M, Co, Ci);
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    float* partial_b = db ? partial + (size_t)p.nblk * Co * Ci : nullptr;
    if (int rc = wgrad_launch(G, X, M, Co, Ci, p, partial, partial_b, st)) return rc;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)cdiv((int64_t)Co * Ci, 64)), dim3(256), 0, st, partial, p.nblk,
                       Co * Ci, dW);
    CRF_LAUNCH_CHECK();
    if (db) {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)cdiv((int64_t)Co, 64)), dim3(256), 0, st, partial_b, p.nblk,
                           Co, db);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}
