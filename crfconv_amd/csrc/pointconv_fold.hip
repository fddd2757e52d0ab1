// PointConv, the small kernels around the edge passes: the fixed-order float64 sums of block-partial rows, the rel-pos moments of a
// neighbour table with their finishers, and the single-workgroup BatchNorm folds (fold1 / fold2 and their backward forms).
#include "pointconv_common.hpp"
#include "reduce64_body.hpp"

namespace crf {

// ------------------------------------------------------------------ generic partial reduction
// out[slot] = sum_b partial[b][slot] in double, fixed order: one wavefront per slot, lane l sums
// blocks l, l+64, ... then a shuffle tree (same result every run).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial,
                                                              int64_t nblk, int nslots,
                                                              double* __restrict__ out) {
    const int slot = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= nslots) return;
    double a = 0.0;
    for (int64_t b = lane; b < nblk; b += WAVE) a += (double)partial[b * nslots + slot];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
    if (lane == 0) out[slot] = a;
}

__global__ __launch_bounds__(256) void reduce_partials_d_kernel(const double* __restrict__ partial,
                                                                int64_t nblk, int nslots,
                                                                double* __restrict__ out) {
    const int slot = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= nslots) return;
    double a = 0.0;
    for (int64_t b = lane; b < nblk; b += WAVE) a += partial[b * nslots + slot];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
    if (lane == 0) out[slot] = a;
}

// (table and body: reduce64_body.hpp)
__global__ __launch_bounds__(256) void reduce_jobs_f64_kernel(const Reduce64Table t) { reduce_jobs_f64_body(t, blockIdx.x); }

// ------------------------------------------------------------------ rel-pos moments
__device__ __forceinline__ void moments_block(const float* __restrict__ pos_src, const float* __restrict__ pos_tgt,
                                              const int32_t* __restrict__ idx, int K, int64_t m_tgt, int64_t blk,
                                              float* __restrict__ partial_row) {
    __shared__ float sred[PWAVES][9];
    const int64_t i = blk * 256 + threadIdx.x;
    float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < m_tgt) {
        const float px = pos_tgt[3 * i], py = pos_tgt[3 * i + 1], pz = pos_tgt[3 * i + 2];
        for (int k = 0; k < K; ++k) {
            const int64_t j = idx[i * K + k];
            if (j < 0) continue;                       // "no neighbour" (padded variable-degree table)
            const float rx = px - pos_src[3 * j], ry = py - pos_src[3 * j + 1], rz = pz - pos_src[3 * j + 2];
            a[0] += rx; a[1] += ry; a[2] += rz;
            a[3] = fmaf(rx, rx, a[3]); a[4] = fmaf(rx, ry, a[4]); a[5] = fmaf(rx, rz, a[5]);
            a[6] = fmaf(ry, ry, a[6]); a[7] = fmaf(ry, rz, a[7]); a[8] = fmaf(rz, rz, a[8]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const float t = wave_sum(a[n]);
        if (lane == 0) sred[wave][n] = t;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < PWAVES; ++w) t += sred[w][threadIdx.x];
        partial_row[threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ pos_src,
                                                      const float* __restrict__ pos_tgt,
                                                      const int32_t* __restrict__ idx, int K,
                                                      int64_t m_tgt, float* __restrict__ partial) {
    moments_block(pos_src, pos_tgt, idx, K, m_tgt, blockIdx.x, partial + (int64_t)blockIdx.x * 9);
}

// The moments of SEVERAL tables (a batch refresh recomputes them for every PointConv layer's table: nine pairs of launches one
// by one): the same per-workgroup partials and the same finishing order per table, two launches for all of them.
constexpr int MB_MAX = 16;
struct MomentsBatch {
    const float* pos_src[MB_MAX];
    const float* pos_tgt[MB_MAX];
    const int32_t* idx[MB_MAX];
    double* mean[MB_MAX];
    double* cov[MB_MAX];
    double* packed[MB_MAX];
    float* mean32[MB_MAX];
    double n_edges[MB_MAX];
    int K[MB_MAX], m_tgt[MB_MAX];
    int blk_base[MB_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(256) void moments_batched_kernel(const MomentsBatch t, float* __restrict__ partial) {
    int lo = 0, hi = t.njobs;                          // largest j with blk_base[j] <= blockIdx.x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.blk_base[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    moments_block(t.pos_src[lo], t.pos_tgt[lo], t.idx[lo], t.K[lo], t.m_tgt[lo], (int)blockIdx.x - t.blk_base[lo],
                  partial + (int64_t)blockIdx.x * 9);
}

// (declared in pointconv_common.hpp: the edge passes of the other two units finish their block partials with these)
int reduce_partials(const float* partial, int64_t nblk, int nslots, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv(nslots, 256 / WAVE)), dim3(256), 0, st, partial,
                       nblk, nslots, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
int reduce_partials_d(const double* partial, int64_t nblk, int nslots, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_partials_d_kernel, dim3((unsigned)cdiv(nslots, 256 / WAVE)), dim3(256), 0, st, partial,
                       nblk, nslots, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

}  // namespace crf

using namespace crf;

// The nine block-partial sums of moments_kernel -> mean [3], covariance [3, 3], packed {mean, cov} [12] (float64) and the mean in
// float32, in ONE single-workgroup launch: slot sums exactly as reduce_partials_kernel forms them (one wavefront per slot, lane l
// takes blocks l, l + 64, ..., shuffle tree), then mean = S1 / n, cov = S2 / n - mean mean^T with every operation rounded on its
// own (what the chain of framework ops this replaces computed: ~15 launches and, on a refresh, four copies per table).
__device__ __forceinline__ void moments_finish_block(const float* __restrict__ partial, int64_t nblk, double n_edges,
                                                     double* __restrict__ mean, double* __restrict__ cov,
                                                     double* __restrict__ packed, float* __restrict__ mean32) {
    __shared__ double s_sum[9];
    const int slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (slot < 9) {
        double a = 0.0;
        for (int64_t b = lane; b < nblk; b += WAVE) a += (double)partial[b * 9 + slot];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
        if (lane == 0) s_sum[slot] = a;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 12) return;
    double v;
    if (t < 3) {
        v = s_sum[t] / n_edges;
    } else {
        const int a = (t - 3) / 3, b = (t - 3) % 3;
        // second moments arrive as the upper triangle xx xy xz yy yz zz (index arithmetic, not a table: no private segment,
        // which a replayed hipGraph does not survive on ROCm 7.2 -- DESIGN.md 5b)
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int tri = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
        const double sec = s_sum[3 + tri] / n_edges;
        v = dadd_rn(sec, -dmul_rn(s_sum[a] / n_edges, s_sum[b] / n_edges));
    }
    packed[t] = v;
    if (t < 3) { mean[t] = v; mean32[t] = (float)v; }
    else cov[t - 3] = v;
}
__global__ __launch_bounds__(1024) void moments_finish_kernel(const float* __restrict__ partial, int64_t nblk, double n_edges,
                                                              double* __restrict__ mean, double* __restrict__ cov,
                                                              double* __restrict__ packed, float* __restrict__ mean32) {
    moments_finish_block(partial, nblk, n_edges, mean, cov, packed, mean32);
}
__global__ __launch_bounds__(1024) void moments_finish_batched_kernel(const MomentsBatch t, const float* __restrict__ partial) {
    const int j = blockIdx.x;
    moments_finish_block(partial + (int64_t)t.blk_base[j] * 9, t.blk_base[j + 1] - t.blk_base[j], t.n_edges[j], t.mean[j], t.cov[j],
                         t.packed[j], t.mean32[j]);
}

extern "C" int crfconv_pointconv_moments_packed(const float* pos_src, const float* pos_tgt, const int32_t* idx32, int K,
                                                int64_t m_tgt, double n_edges, double* mean, double* cov, double* packed,
                                                float* mean32, void* workspace, size_t workspace_bytes,
                                                crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, 4)) return rc;
    CRF_REQUIRE(pos_src && pos_tgt && idx32 && mean && cov && packed && mean32 && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n_edges > 0.0, CRF_ERR_ARG, "n_edges must be positive");
    const int64_t nblk = cdiv(m_tgt, 256);
    CRF_REQUIRE(workspace_bytes >= sizeof(float) * 9 * (size_t)nblk, CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)nblk), dim3(256), 0, st, pos_src, pos_tgt, idx32, K, m_tgt, partial);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(1024), 0, st, partial, nblk, n_edges, mean, cov, packed, mean32);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" size_t crfconv_pointconv_moments_batched_workspace(const crf_moments_job* jobs, int njobs) {
    if (!jobs || njobs < 1) return 0;
    int64_t nblk = 0;
    for (int j = 0; j < njobs; ++j) nblk += cdiv(jobs[j].m_tgt, 256);
    return sizeof(float) * 9 * (size_t)nblk;
}

// crfconv_pointconv_moments_packed for up to 16 tables in two launches: identical outputs (same partials, same order).
extern "C" int crfconv_pointconv_moments_batched(const crf_moments_job* jobs, int njobs, void* workspace, size_t workspace_bytes,
                                                 crf_stream_t stream) {
    CRF_REQUIRE(jobs && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 1 && njobs <= MB_MAX, CRF_ERR_ARG, "njobs=%d outside [1, %d]", njobs, MB_MAX);
    CRF_REQUIRE(workspace_bytes >= crfconv_pointconv_moments_batched_workspace(jobs, njobs), CRF_ERR_WORKSPACE, "workspace too small");
    MomentsBatch t;
    int64_t nblk = 0;
    for (int j = 0; j <= MB_MAX; ++j) {
        t.blk_base[j] = (int)nblk;
        if (j < njobs) {
            const crf_moments_job& jb = jobs[j];
            if (int rc = check_pc(jb.m_tgt, jb.K, 4)) return rc;
            CRF_REQUIRE(jb.pos_src && jb.pos_tgt && jb.idx32 && jb.mean && jb.cov && jb.packed && jb.mean32, CRF_ERR_ARG,
                        "job %d: null pointer", j);
            CRF_REQUIRE(jb.n_edges > 0.0 && jb.m_tgt < ((int64_t)1 << 31), CRF_ERR_ARG, "job %d: bad size", j);
            t.pos_src[j] = jb.pos_src; t.pos_tgt[j] = jb.pos_tgt; t.idx[j] = jb.idx32; t.mean[j] = jb.mean; t.cov[j] = jb.cov;
            t.packed[j] = jb.packed; t.mean32[j] = jb.mean32; t.n_edges[j] = jb.n_edges; t.K[j] = jb.K; t.m_tgt[j] = (int)jb.m_tgt;
            nblk += cdiv(jb.m_tgt, 256);
            CRF_REQUIRE(nblk < ((int64_t)1 << 31), CRF_ERR_UNSUPPORTED, "batch too large");
        } else if (j < MB_MAX) {
            t.pos_src[j] = nullptr; t.pos_tgt[j] = nullptr; t.idx[j] = nullptr; t.mean[j] = nullptr; t.cov[j] = nullptr;
            t.packed[j] = nullptr; t.mean32[j] = nullptr; t.n_edges[j] = 1.0; t.K[j] = 1; t.m_tgt[j] = 0;
        }
    }
    t.njobs = njobs;
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(moments_batched_kernel, dim3((unsigned)nblk), dim3(256), 0, st, t, partial);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(moments_finish_batched_kernel, dim3((unsigned)njobs), dim3(1024), 0, st, t, (const float*)partial);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_reduce_jobs_f64(const crf_reduce64_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j0 = 0; j0 < njobs; j0 += R64_MAX) {
        Reduce64Table t;
        const int n = njobs - j0 < R64_MAX ? njobs - j0 : R64_MAX;
        int64_t waves = 0;
        for (int j = 0; j <= R64_MAX; ++j) {
            t.wave_base[j] = (int)waves;
            if (j < n) {
                const crf_reduce64_job& jb = jobs[j0 + j];
                CRF_REQUIRE(jb.partial && jb.out && jb.nblk > 0 && jb.nblk < ((int64_t)1 << 31) && jb.nslots > 0, CRF_ERR_ARG,
                            "job %d is malformed", j0 + j);
                t.partial[j] = jb.partial; t.out[j] = jb.out; t.is_float[j] = jb.is_float; t.nblk[j] = (int)jb.nblk; t.nslots[j] = jb.nslots;
                waves += jb.nslots;
                CRF_REQUIRE(waves < ((int64_t)1 << 30), CRF_ERR_UNSUPPORTED, "too many slots in one batch");
            } else if (j < R64_MAX) {
                t.partial[j] = nullptr; t.out[j] = nullptr; t.is_float[j] = 0; t.nblk[j] = 0; t.nslots[j] = 0;
            }
        }
        t.njobs = n;
        hipLaunchKernelGGL(reduce_jobs_f64_kernel, dim3((unsigned)cdiv(waves, 256 / WAVE)), dim3(256), 0, st, t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

// ====================================================================== BatchNorm folding (tiny, one block)
// The weight MLP's two BatchNorms are folded into per-channel affine coefficients.  BN-1 sits directly on
// Linear(3 -> d) of rel = p_i - p_j, so its batch statistics are ANALYTIC in the first two moments of rel:
//   mean1[c] = w_c . mu,   var1[c] = w_c^T Sigma w_c      (mu [3], Sigma [3,3] from crfconv_pointconv_moments_packed)
// and so is its backward.  These kernels replace ~60 tiny framework launches per convolution.
namespace crf {

// mom = {mu[3], Sigma[9]} float64.  aux1 [3, d] float64 out = {a = gamma*rstd, mean1, var1}.
__device__ __forceinline__ void fold1_body(const float* __restrict__ W1, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, const double* __restrict__ mom,
                                           double n_edges, float* __restrict__ run_mean,
                                           float* __restrict__ run_var, float momentum, float eps,
                                           int use_batch, int d, float* __restrict__ A1,
                                           float* __restrict__ b1, double* __restrict__ aux1) {
    const int c = threadIdx.x;
    if (c >= d) return;
    const double w[3] = {W1[3 * c], W1[3 * c + 1], W1[3 * c + 2]};
    double mean, var;
    if (use_batch) {
        mean = w[0] * mom[0] + w[1] * mom[1] + w[2] * mom[2];
        var = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) var += w[a] * mom[3 + 3 * a + b] * w[b];
        if (var < 0.0) var = 0.0;
        if (run_mean != nullptr) {
            const double unb = n_edges > 1.0 ? var * (n_edges / (n_edges - 1.0)) : var;
            run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mean);
            run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
        }
    } else {
        mean = run_mean[c];
        var = run_var[c];
    }
    const double a = (double)gamma[c] / sqrt(var + (double)eps);
    A1[3 * c] = (float)(a * w[0]);
    A1[3 * c + 1] = (float)(a * w[1]);
    A1[3 * c + 2] = (float)(a * w[2]);
    b1[c] = (float)((double)beta[c] - a * mean);
    aux1[c] = a;
    aux1[d + c] = mean;
    aux1[2 * d + c] = var;
}

__global__ __launch_bounds__(128) void fold1_kernel(const float* __restrict__ W1, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const double* __restrict__ mom,
                                                    double n_edges, float* __restrict__ run_mean,
                                                    float* __restrict__ run_var, float momentum, float eps,
                                                    int use_batch, int d, float* __restrict__ A1,
                                                    float* __restrict__ b1, double* __restrict__ aux1) {
    fold1_body(W1, gamma, beta, mom, n_edges, run_mean, run_var, momentum, eps, use_batch, d, A1, b1, aux1);
}

// fold1 of ALL PointConv layers of a network in one launch (a workgroup per layer): its inputs -- the weight MLP's first
// layer and the rel-pos moments of the layer's table -- are known before the forward pass starts.
constexpr int F1F_MAX = 24;
struct Fold1Table {
    crf_fold1_job job[F1F_MAX];
};
__global__ __launch_bounds__(128) void fold1_batched_kernel(const Fold1Table t) {
    const crf_fold1_job& j = t.job[blockIdx.x];
    fold1_body(j.W1, j.gamma1, j.beta1, j.mom, j.n_edges, j.run_mean, j.run_var, j.momentum, j.eps, j.use_batch, j.d, j.A1, j.b1,
               j.aux1);
}

// dA1b1 [d, 4] float64 = {dA1[c][0..2], db1[c]}  ->  dW1 [d,3], dgamma1, dbeta1
__device__ __forceinline__ void fold1_bwd_body(const float* __restrict__ W1, const float* __restrict__ gamma,
                                               const double* __restrict__ mom, const double* __restrict__ aux1,
                                               const double* __restrict__ dA1b1, float eps, int use_batch,
                                               int d, float* __restrict__ dW1, float* __restrict__ dgamma,
                                               float* __restrict__ dbeta, const double* __restrict__ dW2_f64,
                                               float* __restrict__ dW2_f32) {
    if (dW2_f64 != nullptr)                 // the float64 accumulator of bwd_params -> the float32 gradient (no cast launch)
        for (int i = threadIdx.x; i < d * d; i += 128) dW2_f32[i] = (float)dW2_f64[i];
    const int c = threadIdx.x;
    if (c >= d) return;
    const double w[3] = {W1[3 * c], W1[3 * c + 1], W1[3 * c + 2]};
    const double a = aux1[c], mean = aux1[d + c], var = aux1[2 * d + c];
    const double r = 1.0 / sqrt(var + (double)eps);
    const double dA[3] = {dA1b1[4 * c], dA1b1[4 * c + 1], dA1b1[4 * c + 2]};
    const double db = dA1b1[4 * c + 3];
    const double da = dA[0] * w[0] + dA[1] * w[1] + dA[2] * w[2] - db * mean;   // A = a w, b = beta - a mean
    dgamma[c] = (float)(da * r);
    dbeta[c] = (float)db;
    double dw[3] = {a * dA[0], a * dA[1], a * dA[2]};
    if (use_batch) {
        const double dv = -0.5 * da * (double)gamma[c] * r * r * r;             // a = gamma (var + eps)^-1/2
        for (int k = 0; k < 3; ++k) {
            double sw = 0.0;
            for (int b = 0; b < 3; ++b) sw += mom[3 + 3 * k + b] * w[b];         // (Sigma w)_k, Sigma symmetric
            dw[k] += -db * a * mom[k] + dv * 2.0 * sw;                           // through mean1 and var1
        }
    }
    dW1[3 * c] = (float)dw[0];
    dW1[3 * c + 1] = (float)dw[1];
    dW1[3 * c + 2] = (float)dw[2];
}

__global__ __launch_bounds__(128) void fold1_bwd_kernel(const float* __restrict__ W1, const float* __restrict__ gamma,
                                                        const double* __restrict__ mom, const double* __restrict__ aux1,
                                                        const double* __restrict__ dA1b1, float eps, int use_batch,
                                                        int d, float* __restrict__ dW1, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, const double* __restrict__ dW2_f64,
                                                        float* __restrict__ dW2_f32) {
    fold1_bwd_body(W1, gamma, mom, aux1, dA1b1, eps, use_batch, d, dW1, dgamma, dbeta, dW2_f64, dW2_f32);
}

// The same for ALL PointConv layers of a backward pass in one launch (a workgroup per layer): nothing in the pass waits for
// dW1 / dgamma1 / dbeta1, so the caller queues the jobs and runs them once at the end (ops.deferred_weight_grads).
constexpr int F1_MAX = 24;
struct Fold1BwdTable {
    crf_fold1_bwd_job job[F1_MAX];
};
__global__ __launch_bounds__(128) void fold1_bwd_batched_kernel(const Fold1BwdTable t) {
    const crf_fold1_bwd_job& j = t.job[blockIdx.x];
    fold1_bwd_body(j.W1, j.gamma1, j.mom, j.aux1, j.dA1b1, j.eps, j.use_batch, j.d, j.dW1, j.dgamma1, j.dbeta1, j.dW2_f64,
                   j.dW2_f32);
}

// stats [2, d] float64 = {sum(h2 - shift), sum (h2 - shift)^2}  ->  a2, b2; aux2 [2, d] = {mean2, rstd2}
__global__ __launch_bounds__(128) void fold2_kernel(const double* __restrict__ stats, const float* __restrict__ shift,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    double n_edges, float* __restrict__ run_mean,
                                                    float* __restrict__ run_var, float momentum, float eps,
                                                    int use_batch, int d, float* __restrict__ a2,
                                                    float* __restrict__ b2, double* __restrict__ aux2) {
    const int c = threadIdx.x;
    if (c >= d) return;
    double mean, var;
    if (use_batch) {
        const double m1 = stats[c] / n_edges;
        mean = (double)shift[c] + m1;
        var = stats[d + c] / n_edges - m1 * m1;
        if (var < 0.0) var = 0.0;
        if (run_mean != nullptr) {
            const double unb = n_edges > 1.0 ? var * (n_edges / (n_edges - 1.0)) : var;
            run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mean);
            run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
        }
    } else {
        mean = run_mean[c];
        var = run_var[c];
    }
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[c] * rstd;
    a2[c] = (float)a;
    b2[c] = (float)((double)beta[c] - a * mean);
    aux2[c] = mean;
    aux2[d + c] = rstd;
}

// red [2, d] float64 = {sum g_w, sum g_w (h2 - shift)}  ->  dgamma2, dbeta2 and the coefficients of
// g_h2 = ca g_w + cb h2 + cc  (BatchNorm backward; eval: ca = gamma rstd, cb = cc = 0)
__global__ __launch_bounds__(128) void fold2_bwd_kernel(const double* __restrict__ red, const float* __restrict__ shift,
                                                        const double* __restrict__ aux2, const float* __restrict__ gamma,
                                                        double n_edges, int use_batch, int d, float* __restrict__ ca,
                                                        float* __restrict__ cb, float* __restrict__ cc,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = threadIdx.x;
    if (c >= d) return;
    fold2_bwd_coef(c, d, red[c], red[d + c], shift, aux2, gamma, n_edges, use_batch, ca, cb, cc, dgamma, dbeta);
}

}  // namespace crf

extern "C" int crfconv_pointconv_fold1(const float* W1, const float* gamma1, const float* beta1, const double* mom,
                                       double n_edges, float* run_mean, float* run_var, float momentum, float eps,
                                       int use_batch, int d, float* A1, float* b1, double* aux1, crf_stream_t stream) {
    CRF_REQUIRE(W1 && gamma1 && beta1 && mom && A1 && b1 && aux1, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(d >= 1 && d <= 128, CRF_ERR_UNSUPPORTED, "d=%d outside [1, 128]", d);
    CRF_REQUIRE(use_batch || (run_mean && run_var), CRF_ERR_ARG, "eval mode needs running statistics");
    hipLaunchKernelGGL(fold1_kernel, dim3(1), dim3(128), 0, as_stream(stream), W1, gamma1, beta1, mom, n_edges, run_mean,
                       run_var, momentum, eps, use_batch, d, A1, b1, aux1);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_pointconv_fold1_batched(const crf_fold1_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    for (int j = 0; j < njobs; ++j) {
        const crf_fold1_job& b = jobs[j];
        CRF_REQUIRE(b.W1 && b.gamma1 && b.beta1 && b.mom && b.A1 && b.b1 && b.aux1, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(b.d >= 1 && b.d <= 128, CRF_ERR_UNSUPPORTED, "job %d: d=%d outside [1, 128]", j, b.d);
        CRF_REQUIRE(b.use_batch || (b.run_mean && b.run_var), CRF_ERR_ARG, "job %d: eval mode needs running statistics", j);
    }
    for (int j0 = 0; j0 < njobs; j0 += F1F_MAX) {
        Fold1Table t;
        const int n = njobs - j0 < F1F_MAX ? njobs - j0 : F1F_MAX;
        for (int j = 0; j < F1F_MAX; ++j) t.job[j] = jobs[j0 + (j < n ? j : 0)];
        hipLaunchKernelGGL(fold1_batched_kernel, dim3((unsigned)n), dim3(128), 0, as_stream(stream), t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" int crfconv_pointconv_fold1_bwd(const float* W1, const float* gamma1, const double* mom, const double* aux1,
                                           const double* dA1b1, float eps, int use_batch, int d, float* dW1,
                                           float* dgamma1, float* dbeta1, const double* dW2_f64, float* dW2_f32,
                                           crf_stream_t stream) {
    CRF_REQUIRE(W1 && gamma1 && mom && aux1 && dA1b1 && dW1 && dgamma1 && dbeta1, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE((dW2_f64 == nullptr) == (dW2_f32 == nullptr), CRF_ERR_ARG, "dW2_f64 / dW2_f32: both or neither");
    CRF_REQUIRE(d >= 1 && d <= 128, CRF_ERR_UNSUPPORTED, "d=%d outside [1, 128]", d);
    hipLaunchKernelGGL(fold1_bwd_kernel, dim3(1), dim3(128), 0, as_stream(stream), W1, gamma1, mom, aux1, dA1b1, eps,
                       use_batch, d, dW1, dgamma1, dbeta1, dW2_f64, dW2_f32);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_pointconv_fold1_bwd_batched(const crf_fold1_bwd_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    for (int j = 0; j < njobs; ++j) {
        const crf_fold1_bwd_job& b = jobs[j];
        CRF_REQUIRE(b.W1 && b.gamma1 && b.mom && b.aux1 && b.dA1b1 && b.dW1 && b.dgamma1 && b.dbeta1, CRF_ERR_ARG,
                    "job %d: null pointer", j);
        CRF_REQUIRE((b.dW2_f64 == nullptr) == (b.dW2_f32 == nullptr), CRF_ERR_ARG, "job %d: dW2_f64 / dW2_f32: both or neither", j);
        CRF_REQUIRE(b.d >= 1 && b.d <= 128, CRF_ERR_UNSUPPORTED, "job %d: d=%d outside [1, 128]", j, b.d);
    }
    for (int j0 = 0; j0 < njobs; j0 += F1_MAX) {
        Fold1BwdTable t;
        const int n = njobs - j0 < F1_MAX ? njobs - j0 : F1_MAX;
        for (int j = 0; j < n; ++j) t.job[j] = jobs[j0 + j];
        for (int j = n; j < F1_MAX; ++j) t.job[j] = jobs[j0];
        hipLaunchKernelGGL(fold1_bwd_batched_kernel, dim3((unsigned)n), dim3(128), 0, as_stream(stream), t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" int crfconv_pointconv_fold2(const double* stats, const float* shift, const float* gamma2, const float* beta2,
                                       double n_edges, float* run_mean, float* run_var, float momentum, float eps,
                                       int use_batch, int d, float* a2, float* b2, double* aux2, crf_stream_t stream) {
    CRF_REQUIRE(gamma2 && beta2 && a2 && b2 && aux2 && (!use_batch || (stats && shift)), CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(d >= 1 && d <= 128, CRF_ERR_UNSUPPORTED, "d=%d outside [1, 128]", d);
    CRF_REQUIRE(use_batch || (run_mean && run_var), CRF_ERR_ARG, "eval mode needs running statistics");
    hipLaunchKernelGGL(fold2_kernel, dim3(1), dim3(128), 0, as_stream(stream), stats, shift, gamma2, beta2, n_edges,
                       run_mean, run_var, momentum, eps, use_batch, d, a2, b2, aux2);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_pointconv_fold2_bwd(const double* red, const float* shift, const double* aux2,
                                           const float* gamma2, double n_edges, int use_batch, int d, float* ca,
                                           float* cb, float* cc, float* dgamma2, float* dbeta2, crf_stream_t stream) {
    CRF_REQUIRE(red && shift && aux2 && gamma2 && ca && cb && cc && dgamma2 && dbeta2, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(d >= 1 && d <= 128, CRF_ERR_UNSUPPORTED, "d=%d outside [1, 128]", d);
    hipLaunchKernelGGL(fold2_bwd_kernel, dim3(1), dim3(128), 0, as_stream(stream), red, shift, aux2, gamma2, n_edges,
                       use_batch, d, ca, cb, cc, dgamma2, dbeta2);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
