// BatchNorm-2 of a PointConv layer folded from the statistics of its edge pass, and the combine
//   out = a2 U + (a2 shift + b2) V
// of the training forward (pointconv.hip: uvstats_body leaves U, V, stats and shift).  ONE arithmetic for every kernel that forms
// `out`: uv_combine_kernel (the elementwise pass), and the Linear kernels that form it while they load their operand -- lin_out of the
// ResNet block is the only forward reader of `out`, so the pass of its own disappears (linear_fwd.hpp, gemm_stats.hip, mlp_small.hip).  Every consumer
// derives bit-identical a2, b2, mean, rstd and the same `out`.
#pragma once

#include "common.hpp"

namespace crf {

// What a consumer needs to form `out` itself (U travels as the kernel's operand pointer).  Passed by value in the kernel arguments.
struct UvFold {
    const float* V = nullptr;         // [m, d]
    const double* stats = nullptr;    // [2][d]: sum (h2 - shift), sum (h2 - shift)^2 over the edges
    const float* shift = nullptr;     // [d]
    const float* gamma = nullptr;     // BatchNorm-2 weight / bias
    const float* beta = nullptr;
    double n_edges = 0.0;
    float* run_mean = nullptr;        // running statistics (both or neither), advanced by the publishing workgroup
    float* run_var = nullptr;
    float momentum = 0.f, eps = 0.f;
    float* a2 = nullptr;              // [d], [d], [2][d] = {mean, rstd}: published for the backward kernels
    float* b2 = nullptr;
    double* aux2 = nullptr;
    float* out = nullptr;             // [m, d]: stored by the workgroups of the first column group
};

struct UvCoef {
    float a, b, sh;                   // a2, b2, shift of the channel
    double mean, rstd, var;
};

// host side: the C record (crf_uv_fold, include/crfconv_amd.h) checked and as kernel arguments
inline bool uv_fold_complete(const crf_uv_fold* f) {
    return f && f->U && f->V && f->stats && f->shift && f->gamma2 && f->beta2 && f->a2 && f->b2 && f->aux2 && f->out &&
           (f->run_mean == nullptr) == (f->run_var == nullptr);
}
inline UvFold uv_fold_args(const crf_uv_fold* f) {
    UvFold uv;
    uv.V = f->V; uv.stats = f->stats; uv.shift = f->shift; uv.gamma = f->gamma2; uv.beta = f->beta2; uv.n_edges = f->n_edges;
    uv.run_mean = f->run_mean; uv.run_var = f->run_var; uv.momentum = f->momentum; uv.eps = f->eps;
    uv.a2 = f->a2; uv.b2 = f->b2; uv.aux2 = f->aux2; uv.out = f->out;
    return uv;
}

// a2 = gamma rstd, b2 = beta - a2 mean of channel c (d channels) from the edge statistics
__device__ __forceinline__ UvCoef uv_coef(int c, int d, const double* __restrict__ stats, const float* __restrict__ shift,
                                          const float* __restrict__ gamma, const float* __restrict__ beta, double n_edges, float eps) {
    UvCoef k;
    const double m1 = stats[c] / n_edges;
    k.mean = (double)shift[c] + m1;
    double var = stats[d + c] / n_edges - m1 * m1;
    if (var < 0.0) var = 0.0;
    k.var = var;
    k.rstd = 1.0 / sqrt(var + (double)eps);
    const double aa = (double)gamma[c] * k.rstd;
    k.a = (float)aa;
    k.b = (float)((double)beta[c] - aa * k.mean);
    k.sh = shift[c];
    return k;
}

// one thread per channel of ONE workgroup of the launch: a2 / b2 / aux2 = {mean, rstd} for the backward, the running statistics
__device__ __forceinline__ void uv_publish(int c, int d, const UvCoef& k, double n_edges, float* __restrict__ run_mean,
                                           float* __restrict__ run_var, float momentum, float* __restrict__ a2_out,
                                           float* __restrict__ b2_out, double* __restrict__ aux2) {
    a2_out[c] = k.a;
    b2_out[c] = k.b;
    aux2[c] = k.mean;
    aux2[d + c] = k.rstd;
    if (run_mean != nullptr) {
        const double unb = n_edges > 1.0 ? k.var * (n_edges / (n_edges - 1.0)) : k.var;
        run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * k.mean);
        run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
    }
}

// the coefficient of V: a2 shift + b2
__device__ __forceinline__ float uv_vcoef(const UvCoef& k) { return fmaf(k.a, k.sh, k.b); }

// out = a2 u + (a2 shift + b2) v, with t = uv_vcoef
__device__ __forceinline__ float uv_out(float a, float t, float u, float v) { return fmaf(a, u, t * v); }
__device__ __forceinline__ float4 uv_out4(const float4 a, const float4 t, const float4 u, const float4 v) {
    return make_float4(uv_out(a.x, t.x, u.x, v.x), uv_out(a.y, t.y, u.y, v.y), uv_out(a.z, t.z, u.z, v.z), uv_out(a.w, t.w, u.w, v.w));
}

}  // namespace crf
