// Weighted softmax cross-entropy with an ignored label (trainval.py:101-104: F.cross_entropy(y_pred, y - 1,
// weight=class_weights, ignore_index=...), mean over the weights of the counted rows).
//   loss = sum_r w[t_r] (lse_r - z[r, t_r]) / sum_r w[t_r]           over rows with t_r != ignore
//   dz[r, c] = g * w[t_r] (exp(z[r,c] - lse_r) - [c == t_r]) / sum w
// Forward: one thread per row (rows of adjacent lanes are adjacent in memory, so a wavefront still reads whole
// cache lines), per-block float64 partials, a last single-block kernel folds them in fixed order.
// The framework's nll_loss kernels reduce on ONE workgroup (126 us forward + 126 us backward at 164 k rows).
#include "common.hpp"
#include "gridsync.hpp"

namespace crf {

constexpr int CE_BLOCK = 256;

__global__ __launch_bounds__(CE_BLOCK) void ce_fwd_kernel(const float* __restrict__ z,
                                                          const int64_t* __restrict__ target,
                                                          const float* __restrict__ weight, int64_t m, int C,
                                                          int64_t ignore_index, int64_t label_shift,
                                                          float* __restrict__ lse,
                                                          double* __restrict__ partial, unsigned* __restrict__ ticket,
                                                          double* __restrict__ sums, float* __restrict__ loss) {
    __shared__ double s_red[3][CE_BLOCK / WAVE];
    __shared__ int s_flag;
    const int64_t r = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x;
    double num = 0.0, den = 0.0, bad = 0.0;
    if (r < m) {
        const float* row = z + r * C;
        float mx = row[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
        const float l = mx + logf(se);
        lse[r] = l;
        const int64_t t = target[r] - label_shift;
        if (t != ignore_index) {
            if (t >= 0 && t < C) {
                const float w = weight ? weight[t] : 1.f;
                num = (double)w * (double)(l - row[t]);
                den = (double)w;
            } else {
                bad = 1.0;                                        // label outside [0, C): counted, not used
            }
        }
    }
    double v[3] = {num, den, bad};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, WAVE);
        if ((threadIdx.x & 63) == 0) s_red[i][threadIdx.x >> 6] = v[i];
    }
    __syncthreads();
    typedef unsigned int ce_u32x2 __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(partial, (int)gridDim.x * 3 * 8);
    if (threadIdx.x < 3) {
        double a = 0.0;
        for (int w = 0; w < CE_BLOCK / WAVE; ++w) a += s_red[threadIdx.x][w];
        // write-through: with a ticket the launch's last workgroup (another CU, maybe another XCD) reads the rows below
        const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
        const ce_u32x2 u = {(unsigned)bits, (unsigned)(bits >> 32)};
        __builtin_amdgcn_raw_buffer_store_b64(u, pr, ((int)blockIdx.x * 3 + (int)threadIdx.x) * 8, 0, 16);
    }
    // "the last workgroup finishes" (gridsync.hpp): ce_finalize_kernel's arithmetic, in its order, without its launch
    if (ticket == nullptr || !last_workgroup(ticket, gridDim.x, &s_flag)) return;
    double t[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < (int)gridDim.x; b += CE_BLOCK)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const ce_u32x2 w2 = __builtin_amdgcn_raw_buffer_load_b64(pr, (b * 3 + i) * 8, 0, 16);
            t[i] += __longlong_as_double((long long)(((unsigned long long)w2.y << 32) | w2.x));
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[i] += __shfl_xor(t[i], o, WAVE);
        if ((threadIdx.x & 63) == 0) s_red[i][threadIdx.x >> 6] = t[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a[3];
        for (int i = 0; i < 3; ++i) a[i] = s_red[i][0] + s_red[i][1] + s_red[i][2] + s_red[i][3];
        sums[0] = a[0]; sums[1] = a[1]; sums[2] = a[2];
        *loss = (float)(a[0] / a[1]);
    }
}

// sums = {sum w nll, sum w, #bad labels}; loss = sums[0] / sums[1] (nan when nothing is counted, like the framework)
__global__ __launch_bounds__(256) void ce_finalize_kernel(const double* __restrict__ partial, int64_t nblk,
                                                          double* __restrict__ sums, float* __restrict__ loss) {
    __shared__ double s_red[3][256 / WAVE];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] += partial[b * 3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, WAVE);
        if ((threadIdx.x & 63) == 0) s_red[i][threadIdx.x >> 6] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a[3];
        for (int i = 0; i < 3; ++i) a[i] = s_red[i][0] + s_red[i][1] + s_red[i][2] + s_red[i][3];
        sums[0] = a[0]; sums[1] = a[1]; sums[2] = a[2];
        *loss = (float)(a[0] / a[1]);
    }
}

// one thread per logit
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ z, const int64_t* __restrict__ target,
                                                     const float* __restrict__ weight, const float* __restrict__ lse,
                                                     const double* __restrict__ sums, const float* __restrict__ gloss,
                                                     int64_t m, int C, int64_t ignore_index, int64_t label_shift,
                                                     float* __restrict__ dz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m * C) return;
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    const int64_t t = target[r] - label_shift;
    float out = 0.f;
    if (t != ignore_index && t >= 0 && t < C) {
        const float w = weight ? weight[t] : 1.f;
        const float scale = (float)((double)gloss[0] * (double)w / sums[1]);
        out = scale * (expf(z[i] - lse[r]) - (c == t ? 1.f : 0.f));
    }
    dz[i] = out;
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_softmax_ce_workspace(int64_t m) {
    return m > 0 ? sizeof(double) * 3 * (size_t)cdiv(m, CE_BLOCK) + 256 : 0;
}

extern "C" int crfconv_softmax_ce_forward(const float* logits, const int64_t* target, const float* weight,
                                          int64_t m, int C, int64_t ignore_index, int64_t label_shift, float* lse,
                                          double* sums, float* loss, void* workspace, size_t workspace_bytes,
                                          unsigned* ticket, crf_stream_t stream) {
    CRF_REQUIRE(logits && target && lse && sums && loss && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(m > 0 && C >= 1 && C <= 4096 && m * C < ((int64_t)1 << 40), CRF_ERR_ARG, "m=%lld C=%d out of range",
                (long long)m, C);
    CRF_REQUIRE(workspace_bytes >= crfconv_softmax_ce_workspace(m), CRF_ERR_WORKSPACE, "workspace too small");
    double* partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    const int64_t nblk = cdiv(m, CE_BLOCK);
    hipStream_t st = as_stream(stream);
    if (nblk * 3 * 8 >= ((int64_t)1 << 31)) ticket = nullptr;             // (the partial rows are addressed through a 32-bit buffer descriptor)
    hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)nblk), dim3(CE_BLOCK), 0, st, logits, target, weight, m, C,
                       ignore_index, label_shift, lse, partial, ticket, sums, loss);
    CRF_LAUNCH_CHECK();
    if (ticket == nullptr) {                                               // no ticket words: the fold as a launch of its own
        hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nblk, sums, loss);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" int crfconv_softmax_ce_backward(const float* logits, const int64_t* target, const float* weight,
                                           const float* lse, const double* sums, const float* grad_loss, int64_t m,
                                           int C, int64_t ignore_index, int64_t label_shift, float* dlogits,
                                           crf_stream_t stream) {
    CRF_REQUIRE(logits && target && lse && sums && grad_loss && dlogits, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(m > 0 && C >= 1 && C <= 4096 && m * C < ((int64_t)1 << 40), CRF_ERR_ARG, "m=%lld C=%d out of range",
                (long long)m, C);
    hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)cdiv(m * C, 256)), dim3(256), 0, as_stream(stream), logits,
                       target, weight, lse, sums, grad_loss, m, C, ignore_index, label_shift, dlogits);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
