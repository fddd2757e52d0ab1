// The optimizer steps over ONE flat float32 parameter vector (crfconv_amd.optim: FlatSGD, FlatAdam), one launch chain for the
// whole model instead of ~15 multi-tensor ones.  Everything that changes between steps -- the hyper-parameters, Adam's step counter --
// is read from DEVICE memory, so a captured hipGraph of the step follows a scheduler (launch scalars are frozen at capture time).
// Both steps share the guard below: while a sticky failure word is set, the update is skipped.
//
// ====================================================================== SGD (trainval.py:69-72, 105)
// torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov):
//   g = grad * grad_scale + wd * p;  buf = first ? g : mu * buf + (1 - dampening) * g;  g = nesterov ? g + mu * buf : buf;  p -= lr * g
// (momentum == 0: p -= lr * g, buf untouched), hyper = {lr, momentum, dampening, weight_decay, grad_scale} (trainval.py:73
// ExponentialLR rewrites lr between replays).
#include "common.hpp"

namespace crf {
// the sticky failure words a guarded update looks at: the grid-barrier words of every barrier workspace of the device (a step may
// have run eagerly on one stream and as a captured graph on another: each has its own words) and, under data parallelism, the
// REDUCED flag -- a float slot behind the flat gradient bucket that every rank fills with its own state before the all-reduce, so
// that all replicas skip the update of a step in which ANY rank failed (its NaN gradient was summed into everybody's bucket)
constexpr int SGD_MAX_FAIL = 8;
struct SgdGuard {
    const unsigned* words[SGD_MAX_FAIL];
    int nwords;
    const float* reduced;      // may be null
};
__device__ __forceinline__ bool sgd_guard_set(const SgdGuard& gd) {
    bool bad = false;
    for (int i = 0; i < gd.nwords; ++i) bad |= *gd.words[i] != 0u;
    if (gd.reduced != nullptr) bad |= !(*gd.reduced == 0.f);          // (a NaN slot counts as set)
    return bad;
}
// slot = 1 when any of the local words is set, else 0 (one thread: the words are a handful)
__global__ void sgd_guard_publish_kernel(const SgdGuard gd, float* __restrict__ slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        bool bad = false;
        for (int i = 0; i < gd.nwords; ++i) bad |= *gd.words[i] != 0u;
        *slot = bad ? 1.f : 0.f;
    }
}
__global__ __launch_bounds__(256) void sgd_hyper_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ buf, int64_t n,
                                                        const float* __restrict__ hyper, int nesterov, int first,
                                                        const SgdGuard guard) {
    // guard: sticky failure words (gridsync.hpp FW_FAIL) and the rank-reduced flag.  A one-launch kernel whose barrier
    // gave up has NaN-poisoned its outputs, hence the gradient: the update is SKIPPED while any of them is set (uniform scalar
    // loads), so parameters and momentum survive until ops.check_gridsync reports the failure -- also in captured replays
    if (sgd_guard_set(guard)) return;
    // hyper[4] = gradient scale: 1 / world size when the bucket holds the all-reduce SUM of the ranks' gradients (the mean
    // then never exists as a pass of its own over the bucket); 1 otherwise (x * 1.0f is exact)
    const float lr = hyper[0], mu = hyper[1], damp = hyper[2], wd = hyper[3], gs = hyper[4];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float w = p[i];
        float d = fmaf(wd, w, g[i] * gs);
        if (mu != 0.f) {
            const float b = first ? d : fmaf(mu, buf[i], (1.f - damp) * d);
            buf[i] = b;
            d = nesterov ? fmaf(mu, b, d) : b;
        }
        p[i] = fmaf(-lr, d, w);
    }
}
}  // namespace crf

using namespace crf;

static int sgd_guard_of(const unsigned* const* fail_words, int nwords, const float* reduced, crf::SgdGuard& gd) {
    CRF_REQUIRE(nwords >= 0 && nwords <= crf::SGD_MAX_FAIL, CRF_ERR_ARG, "%d failure words (at most %d)", nwords, crf::SGD_MAX_FAIL);
    CRF_REQUIRE(nwords == 0 || fail_words != nullptr, CRF_ERR_ARG, "null pointer");
    for (int i = 0; i < crf::SGD_MAX_FAIL; ++i) gd.words[i] = nullptr;
    for (int i = 0; i < nwords; ++i) {
        CRF_REQUIRE(fail_words[i] != nullptr, CRF_ERR_ARG, "failure word %d: null pointer", i);
        gd.words[i] = fail_words[i];
    }
    gd.nwords = nwords;
    gd.reduced = reduced;
    return CRF_OK;
}

extern "C" int crfconv_sgd_step_guarded_all(float* param, const float* grad, float* momentum_buf, int64_t n,
                                            const float* hyper, int nesterov, int first_step,
                                            const unsigned* const* fail_words, int n_fail_words, const float* reduced_flag,
                                            crf_stream_t stream) {
    crf::SgdGuard gd;
    if (int rc = sgd_guard_of(fail_words, n_fail_words, reduced_flag, gd)) return rc;
    CRF_REQUIRE(param && grad && momentum_buf && hyper, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0, CRF_ERR_ARG, "n=%lld <= 0", (long long)n);
    int64_t nb = cdiv(n, 256 * 4);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(crf::sgd_hyper_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), param, grad, momentum_buf,
                       n, hyper, nesterov, first_step, gd);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_sgd_guard_publish(const unsigned* const* fail_words, int n_fail_words, float* slot, crf_stream_t stream) {
    CRF_REQUIRE(slot, CRF_ERR_ARG, "null pointer");
    crf::SgdGuard gd;
    if (int rc = sgd_guard_of(fail_words, n_fail_words, nullptr, gd)) return rc;
    hipLaunchKernelGGL(crf::sgd_guard_publish_kernel, dim3(1), dim3(64), 0, as_stream(stream), gd, slot);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// ====================================================================== Adam / AdamW (trainval.py:66-68)
// torch.optim.Adam (single-tensor, non-capturable path), operation for operation, over ONE flat float32 vector:
//   g = grad * grad_scale * clip_coef;  coupled: g += wd * p;  decoupled (AdamW): p *= 1 - lr * wd
//   m += (g - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;  amsgrad: vmax = max(vmax, v)
//   denom = sqrt(v or vmax) / sqrt(1 - beta2^t) + eps;  p -= (lr / (1 - beta1^t)) * m / denom
// At most three launches per step, none of them the framework's:
//   adam_sqnorm_kernel   (only with max_grad_norm) per-workgroup float64 sums of (grad_scale * g)^2 into a workspace
//   adam_prologue_kernel one workgroup: folds those sums in a fixed order (no floating-point atomics: the norm is bit-reproducible),
//                        reads the guard, advances the DEVICE step counter t -- not on a skipped step -- and writes the step's
//                        coefficients (both bias corrections in float64 from the float64 betas, once per step) to `coef`
//   adam_update_kernel   one grid-stride pass over {p, g, m, v[, vmax]}; every workgroup reads the same coefficients, so no workgroup
//                        can see a counter that another one of the same launch has advanced
// The hyper-parameters {lr, beta1, beta2, eps, weight_decay, grad_scale, max_grad_norm} are 7 doubles in DEVICE memory (the values
// as Python holds them): a captured step follows a scheduler, and t counts replays, which no launch scalar could.
namespace crf {
constexpr int ADAM_BLOCK = 256, ADAM_MAX_BLOCKS = 2048;
enum { AC_SKIP = 0, AC_GS, AC_CLIP, AC_WD, AC_DECAY, AC_OMB1, AC_BETA2, AC_OMB2, AC_BC2S, AC_EPS, AC_STEP, AC_COUNT };

struct AdamCoef {
    float gs, clip, wd, decay, omb1, beta2, omb2, bc2s, eps, step;
};
__device__ __forceinline__ AdamCoef adam_coef_of(const float* __restrict__ c) {
    return AdamCoef{c[AC_GS], c[AC_CLIP], c[AC_WD], c[AC_DECAY], c[AC_OMB1], c[AC_BETA2], c[AC_OMB2], c[AC_BC2S], c[AC_EPS], c[AC_STEP]};
}

template <bool AMS>
__device__ __forceinline__ void adam_elem(float& p, const float gr, float& m, float& v, float& vmax, const AdamCoef& c, const bool decoupled) {
    // every operation rounded on its own, in torch's order (no contraction into FMAs): the vector and the element-by-element form
    // of the kernel then give equal bits, and the float32 reference of the tests is followed operation for operation
#pragma clang fp contract(off)
    float g = gr * c.gs * c.clip;
    if (decoupled) p *= c.decay;
    else g += c.wd * p;
    const float diff = g - m;                                            // Tensor.lerp_: both forms of ATen's lerp
    m = c.omb1 < 0.5f ? m + c.omb1 * diff : g - diff * (1.f - c.omb1);
    v = v * c.beta2;
    v += c.omb2 * g * g;
    float s = v;
    if (AMS) {
        vmax = fmaxf(vmax, v);
        s = vmax;
    }
    const float denom = sqrtf(s) / c.bc2s + c.eps;
    p += (-c.step * m) / denom;
}

// VEC: all operand pointers are 16-byte aligned -- float4 loads and stores over the n / 4 whole quads, the n % 4 tail by the first lanes
// of workgroup 0; otherwise one element per lane (a misaligned view handed to the C entry: correct, slower)
template <bool VEC, bool AMS>
__global__ __launch_bounds__(ADAM_BLOCK) void adam_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, float* __restrict__ vmax, int64_t n,
                                                                 const float* __restrict__ coef, int decoupled) {
    if (coef[AC_SKIP] != 0.f) return;                                    // the prologue saw a failure word: nothing changes
    const AdamCoef c = adam_coef_of(coef);
    const int64_t tid = (int64_t)blockIdx.x * ADAM_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * ADAM_BLOCK;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t q = tid; q < n4; q += stride) {
            float4 P = ld4(p + 4 * q), M = ld4(m + 4 * q), V = ld4(v + 4 * q), X = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 G = ld4(g + 4 * q);
            if (AMS) X = ld4(vmax + 4 * q);
            adam_elem<AMS>(P.x, G.x, M.x, V.x, X.x, c, decoupled != 0);
            adam_elem<AMS>(P.y, G.y, M.y, V.y, X.y, c, decoupled != 0);
            adam_elem<AMS>(P.z, G.z, M.z, V.z, X.z, c, decoupled != 0);
            adam_elem<AMS>(P.w, G.w, M.w, V.w, X.w, c, decoupled != 0);
            st4(p + 4 * q, P); st4(m + 4 * q, M); st4(v + 4 * q, V);
            if (AMS) st4(vmax + 4 * q, X);
        }
    }
    for (int64_t i = (VEC ? (n & ~(int64_t)3) : 0) + tid; i < n; i += stride) {
        float P = p[i], M = m[i], V = v[i], X = AMS ? vmax[i] : 0.f;
        adam_elem<AMS>(P, g[i], M, V, X, c, decoupled != 0);
        p[i] = P; m[i] = M; v[i] = V;
        if (AMS) vmax[i] = X;
    }
}

__device__ __forceinline__ double adam_block_sum(double a, double* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = a;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// partial[b] = sum over workgroup b's elements of (grad_scale * g)^2, float64 (the bucket itself is not rewritten)
template <bool VEC>
__global__ __launch_bounds__(ADAM_BLOCK) void adam_sqnorm_kernel(const float* __restrict__ g, int64_t n, const double* __restrict__ hyper,
                                                                 double* __restrict__ partial) {
    __shared__ double s_red[ADAM_BLOCK / WAVE];
    const float gs = (float)hyper[5];
    const int64_t tid = (int64_t)blockIdx.x * ADAM_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * ADAM_BLOCK;
    double a = 0.0;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t q = tid; q < n4; q += stride) {
            const float4 G = ld4(g + 4 * q);
            const double x = (double)(G.x * gs), y = (double)(G.y * gs), z = (double)(G.z * gs), w = (double)(G.w * gs);
            a += x * x + y * y + z * z + w * w;
        }
    }
    for (int64_t i = (VEC ? (n & ~(int64_t)3) : 0) + tid; i < n; i += stride) {
        const double x = (double)(g[i] * gs);
        a += x * x;
    }
    a = adam_block_sum(a, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

// One workgroup.  partial == nullptr: no clipping (clip_coef = 1, *grad_norm untouched).
__global__ __launch_bounds__(ADAM_BLOCK) void adam_prologue_kernel(const double* __restrict__ hyper, long long* __restrict__ t,
                                                                   float* __restrict__ coef, float* __restrict__ grad_norm,
                                                                   const double* __restrict__ partial, int nblk, const SgdGuard guard) {
    __shared__ double s_red[ADAM_BLOCK / WAVE];
    double a = 0.0;
    if (partial != nullptr) {
        for (int b = threadIdx.x; b < nblk; b += ADAM_BLOCK) a += partial[b];
        a = adam_block_sum(a, s_red);
    }
    if (threadIdx.x != 0) return;
    float clip = 1.f;
    if (partial != nullptr) {
        // torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False): coef = clamp(max_norm / (norm + 1e-6), max=1) in
        // float32; a NaN norm gives a NaN coefficient, an infinite one 0 (exactly as there)
        const float norm = (float)sqrt(a);
        *grad_norm = norm;
        const float cc = (float)hyper[6] / (norm + 1e-6f);
        clip = cc > 1.f ? 1.f : cc;
    }
    if (sgd_guard_set(guard)) {                                          // sticky failure word or reduced flag: the step is skipped,
        coef[AC_SKIP] = 1.f;                                             // t does not advance
        return;
    }
    const long long step = *t + 1;
    *t = step;
    const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    coef[AC_SKIP] = 0.f;
    coef[AC_GS] = (float)hyper[5];
    coef[AC_CLIP] = clip;
    coef[AC_WD] = (float)wd;
    coef[AC_DECAY] = (float)(1.0 - lr * wd);
    coef[AC_OMB1] = (float)(1.0 - b1);
    coef[AC_BETA2] = (float)b2;
    coef[AC_OMB2] = (float)(1.0 - b2);
    coef[AC_BC2S] = (float)sqrt(bc2);
    coef[AC_EPS] = (float)eps;
    coef[AC_STEP] = (float)(lr / bc1);
}
}  // namespace crf

static int adam_blocks(int64_t n) {
    const int64_t nb = cdiv(n, (int64_t)crf::ADAM_BLOCK * 4);
    return (int)(nb > crf::ADAM_MAX_BLOCKS ? crf::ADAM_MAX_BLOCKS : nb);
}

extern "C" size_t crfconv_adam_workspace(int64_t n) { return n > 0 ? sizeof(double) * (size_t)adam_blocks(n) : 0; }

extern "C" size_t crfconv_adam_coef_floats(void) { return (size_t)crf::AC_COUNT; }

extern "C" int crfconv_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                                 const double* hyper, long long* t, float* coef, float* grad_norm, int decoupled, int clip,
                                 void* workspace, size_t workspace_bytes, const unsigned* const* fail_words, int n_fail_words,
                                 const float* reduced_flag, crf_stream_t stream) {
    CRF_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper && t && coef, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0, CRF_ERR_ARG, "n=%lld <= 0", (long long)n);
    const uintptr_t all = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                          reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(max_exp_avg_sq);
    CRF_REQUIRE((all & 3) == 0, CRF_ERR_ARG, "operand vectors must be 4-byte aligned");
    CRF_REQUIRE((reinterpret_cast<uintptr_t>(hyper) & 7) == 0 && (reinterpret_cast<uintptr_t>(t) & 7) == 0, CRF_ERR_ARG,
                "hyper / t must be 8-byte aligned");
    crf::SgdGuard gd;
    if (int rc = sgd_guard_of(fail_words, n_fail_words, reduced_flag, gd)) return rc;
    const int nb = adam_blocks(n);
    hipStream_t st = as_stream(stream);
    double* partial = nullptr;
    if (clip) {
        CRF_REQUIRE(workspace && grad_norm, CRF_ERR_ARG, "null pointer (clipping needs a workspace and grad_norm)");
        CRF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, CRF_ERR_ARG, "workspace must be 8-byte aligned");
        CRF_REQUIRE(workspace_bytes >= crfconv_adam_workspace(n), CRF_ERR_WORKSPACE, "workspace too small");
        partial = static_cast<double*>(workspace);
        if ((reinterpret_cast<uintptr_t>(grad) & 15) == 0)
            hipLaunchKernelGGL(crf::adam_sqnorm_kernel<true>, dim3((unsigned)nb), dim3(crf::ADAM_BLOCK), 0, st, grad, n, hyper, partial);
        else
            hipLaunchKernelGGL(crf::adam_sqnorm_kernel<false>, dim3((unsigned)nb), dim3(crf::ADAM_BLOCK), 0, st, grad, n, hyper, partial);
        CRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(crf::adam_prologue_kernel, dim3(1), dim3(crf::ADAM_BLOCK), 0, st, hyper, t, coef, grad_norm,
                       static_cast<const double*>(partial), nb, gd);
    CRF_LAUNCH_CHECK();
    const bool vec = (all & 15) == 0, ams = max_exp_avg_sq != nullptr;
    const dim3 grid((unsigned)nb), block(crf::ADAM_BLOCK);
    if (vec && ams)
        hipLaunchKernelGGL((crf::adam_update_kernel<true, true>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, coef, decoupled);
    else if (vec)
        hipLaunchKernelGGL((crf::adam_update_kernel<true, false>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, coef, decoupled);
    else if (ams)
        hipLaunchKernelGGL((crf::adam_update_kernel<false, true>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, coef, decoupled);
    else
        hipLaunchKernelGGL((crf::adam_update_kernel<false, false>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, coef, decoupled);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
