// Neighbour pooling over a table -- max (strided ResNet shortcut, point_conv_big.py:74-77), sum, mean and min
// (scatter(x[j], i, reduce=), models/common.py:9-23) -- and nearest up-sampling (row gather, :97-101 /
// continuous_crf_conv_big.py:60), forward and backward.
// One thread per (row, 4-channel quad): 16-byte loads, a row's C/4 quads are adjacent lanes.
#include "common.hpp"

namespace crf {

// AFFINE: the pooled quantity is a x + b per channel (coef = [a | b | ..] rows of C floats: a BatchNorm without activation
// applied while gathering -- the strided shortcut of a ResNet block, models/point_conv_big.py:74-83 -- so the normalised
// fine-level tensor never reaches memory; fmaf(a, x, b) is exactly what bn_apply would have stored).
template <bool AFFINE>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x,
                                                          const int32_t* __restrict__ idx, int K,
                                                          int64_t m_tgt, int C4,
                                                          float* __restrict__ out,
                                                          int32_t* __restrict__ arg,
                                                          const float* __restrict__ coef) {
    const int64_t t = (int64_t)xcd_block_id() * 256 + threadIdx.x;
    if (t >= m_tgt * C4) return;
    const int64_t i = t / C4;
    const int q = (int)(t - i * C4);
    const int32_t* irow = idx + i * K;
    float4 ca = make_float4(1.f, 1.f, 1.f, 1.f), cb = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (AFFINE) { ca = ld4(coef + 4 * q); cb = ld4(coef + 4 * C4 + 4 * q); }
    const float ninf = -__builtin_inff();
    float4 best = make_float4(ninf, ninf, ninf, ninf);
    int4 who = make_int4(-1, -1, -1, -1);
    for (int k0 = 0; k0 < K; k0 += 4) {                         // four neighbours per trip: index entries, then rows
        int jn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) jn[u] = k0 + u < K ? irow[k0 + u] : -1;
        float4 vn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vn[u] = ld4(x + ((int64_t)(jn[u] < 0 ? 0 : jn[u]) * C4 + q) * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (jn[u] < 0) continue;                             // "no neighbour" entry of a padded table
            float4 v = vn[u];
            if constexpr (AFFINE) v = make_float4(fmaf(ca.x, v.x, cb.x), fmaf(ca.y, v.y, cb.y), fmaf(ca.z, v.z, cb.z), fmaf(ca.w, v.w, cb.w));
            const int k = k0 + u;
            if (v.x > best.x || who.x < 0) { best.x = v.x; who.x = k; }
            if (v.y > best.y || who.y < 0) { best.y = v.y; who.y = k; }
            if (v.z > best.z || who.z < 0) { best.z = v.z; who.z = k; }
            if (v.w > best.w || who.w < 0) { best.w = v.w; who.w = k; }
        }
    }
    if (who.x < 0) best = make_float4(0.f, 0.f, 0.f, 0.f);      // empty group -> 0 (scatter_max convention)
    st4(out + t * 4, best);
    *reinterpret_cast<int4*>(arg + t * 4) = who;
}

enum { POOL_SUM = 0, POOL_MEAN = 1, POOL_MAX = 2, POOL_MIN = 3 };

// The other reductions of scatter(x[j], i, reduce=) over the same trip (max is maxpool_fwd_kernel<false>).  Sum: a float accumulator
// from 0 over the valid columns in column order; mean: that sum, then one division by the degree; min: strict <, the first valid
// column that attains it wins (arg as the max writes it).  A row without a valid entry gives 0 (arg -1).  count (may be NULL): the
// row's degree, written by the row's first quad.
template <int REDUCE>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ x,
                                                       const int32_t* __restrict__ idx, int K,
                                                       int64_t m_tgt, int C4,
                                                       float* __restrict__ out,
                                                       int32_t* __restrict__ arg,
                                                       int32_t* __restrict__ count) {
    const int64_t t = (int64_t)xcd_block_id() * 256 + threadIdx.x;
    if (t >= m_tgt * C4) return;
    const int64_t i = t / C4;
    const int q = (int)(t - i * C4);
    const int32_t* irow = idx + i * K;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);              // the running sum, or the running minimum once who >= 0
    int4 who = make_int4(-1, -1, -1, -1);
    int deg = 0;
    for (int k0 = 0; k0 < K; k0 += 4) {                         // four neighbours per trip: index entries, then rows
        int jn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) jn[u] = k0 + u < K ? irow[k0 + u] : -1;
        float4 vn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vn[u] = ld4(x + ((int64_t)(jn[u] < 0 ? 0 : jn[u]) * C4 + q) * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (jn[u] < 0) continue;                             // "no neighbour" entry of a padded table
            const float4 v = vn[u];
            ++deg;
            if constexpr (REDUCE == POOL_MIN) {
                const int k = k0 + u;
                if (v.x < acc.x || who.x < 0) { acc.x = v.x; who.x = k; }
                if (v.y < acc.y || who.y < 0) { acc.y = v.y; who.y = k; }
                if (v.z < acc.z || who.z < 0) { acc.z = v.z; who.z = k; }
                if (v.w < acc.w || who.w < 0) { acc.w = v.w; who.w = k; }
            } else {
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        }
    }
    if constexpr (REDUCE == POOL_MEAN) {
        if (deg > 0) {
            const float n = (float)deg;
            acc = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
        }
    }
    st4(out + t * 4, acc);                                       // (an empty row never left the 0 it started from)
    if constexpr (REDUCE == POOL_MIN) *reinterpret_cast<int4*>(arg + t * 4) = who;
    if (count != nullptr && q == 0) count[i] = deg;
}

// count[i] = valid entries of row i, for the max, whose kernel does not count: one thread per row.
__global__ __launch_bounds__(256) void pool_count_kernel(const int32_t* __restrict__ idx, int K, int64_t m_tgt,
                                                         int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m_tgt) return;
    int deg = 0;
    for (int k = 0; k < K; ++k) deg += idx[i * K + k] >= 0 ? 1 : 0;
    count[i] = deg;
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ gout,
                                                          const int32_t* __restrict__ arg,
                                                          const int32_t* __restrict__ rev_ptr,
                                                          const int32_t* __restrict__ rev_eid, int K,
                                                          int64_t m_src, int C4,
                                                          float* __restrict__ dx) {
    const int64_t t = (int64_t)xcd_block_id() * 256 + threadIdx.x;
    if (t >= m_src * C4) return;
    const int64_t j = t / C4;
    const int q = (int)(t - j * C4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int beg = rev_ptr[j], end = rev_ptr[j + 1];
    // four reverse edges per trip: their edge ids first, then the four (arg, gradient) row pairs -- two dependent memory
    // phases per four edges instead of two per edge; summed in edge order as before
    const int kshift = (K & (K - 1)) == 0 ? __ffs(K) - 1 : -1;
    for (int p = beg; p < end; p += 4) {
        int e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = p + u < end ? rev_eid[p + u] : -1;
        int4 who[4];
        float4 g[4];
        int kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ee = e[u] < 0 ? 0 : e[u];
            const int i = kshift >= 0 ? (ee >> kshift) : (ee / K);
            kk[u] = e[u] < 0 ? -2 : ee - i * K;                 // -2 matches no arg entry
            const int64_t o = ((int64_t)i * C4 + q) * 4;
            who[u] = *reinterpret_cast<const int4*>(arg + o);
            g[u] = ld4(gout + o);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (who[u].x == kk[u]) acc.x += g[u].x;
            if (who[u].y == kk[u]) acc.y += g[u].y;
            if (who[u].z == kk[u]) acc.z += g[u].z;
            if (who[u].w == kk[u]) acc.w += g[u].w;
        }
    }
    st4(dx + t * 4, acc);
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x,
                                                          const int32_t* __restrict__ idx,
                                                          int64_t m_tgt, int C4,
                                                          float* __restrict__ out) {
    const int64_t t = (int64_t)xcd_block_id() * 256 + threadIdx.x;
    if (t >= m_tgt * C4) return;
    const int64_t i = t / C4;
    const int q = (int)(t - i * C4);
    st4(out + t * 4, ld4(x + ((int64_t)idx[i] * C4 + q) * 4));
}

// The backward of the sum and the mean over a table: dx[j] = sum over the reverse row's edges e = i K + k of gout[i] (MEAN: of
// gout[i] / (float)count[i]).  K1: a K = 1 table (ops.gather_rows, nearest up-sampling), whose edge id IS the target row -- its own
// instantiation, so that no division by K enters it.
template <bool K1, bool MEAN>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ gout,
                                                       const int32_t* __restrict__ count,
                                                       const int32_t* __restrict__ rev_ptr,
                                                       const int32_t* __restrict__ rev_eid, int K,
                                                       int64_t m_src, int C4,
                                                       float* __restrict__ dx) {
    const int64_t t = (int64_t)xcd_block_id() * 256 + threadIdx.x;
    if (t >= m_src * C4) return;
    const int64_t j = t / C4;
    const int q = (int)(t - j * C4);
    // A reverse row is summed in edge order in float, 64 edges at a time, and the 64-edge sums are added in double: rows of up to
    // 64 edges (every row of an ordinary up-sampling) get the plain float sum, while a coarse point that a whole cloud
    // up-samples from -- a row of thousands of edges, where one float running sum drifts by 1.3e-6 of the largest gradient at
    // 1031 edges -- stays within a 64-term sum's rounding.
    double tx = 0.0, ty = 0.0, tz = 0.0, tw = 0.0;
    const int beg = rev_ptr[j], end = rev_ptr[j + 1];
    [[maybe_unused]] const int kshift = (K & (K - 1)) == 0 ? __ffs(K) - 1 : -1;
    for (int p0 = beg; p0 < end; p0 += 64) {
        const int pe = min(p0 + 64, end);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = p0; p < pe; p += 4) {            // four reverse edges per trip (ids, then rows), summed in edge order
            int e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = p + u < pe ? rev_eid[p + u] : -1;
            float4 g[4];
            [[maybe_unused]] float cn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int i = e[u] < 0 ? 0 : e[u];
                if constexpr (!K1) i = kshift >= 0 ? (i >> kshift) : (i / K);
                g[u] = ld4(gout + ((int64_t)i * C4 + q) * 4);
                if constexpr (MEAN) cn[u] = (float)count[i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e[u] >= 0) {
                    if constexpr (MEAN) { acc.x += g[u].x / cn[u]; acc.y += g[u].y / cn[u]; acc.z += g[u].z / cn[u]; acc.w += g[u].w / cn[u]; }
                    else { acc.x += g[u].x; acc.y += g[u].y; acc.z += g[u].z; acc.w += g[u].w; }
                }
        }
        tx += acc.x; ty += acc.y; tz += acc.z; tw += acc.w;
    }
    st4(dx + t * 4, make_float4((float)tx, (float)ty, (float)tz, (float)tw));
}

static int check(int64_t rows, int C) {
    CRF_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31), CRF_ERR_ARG, "rows=%lld out of range", (long long)rows);
    CRF_REQUIRE(C > 0 && C % 4 == 0, CRF_ERR_UNSUPPORTED, "channels C=%d must be a positive multiple of 4", C);
    return CRF_OK;
}

// Residual join of the ResNet block (point_conv_big.py:86-88): out = lrelu(a + b, slope); its backward
// g_in = g * (out > 0 ? 1 : slope) serves both addends (slope > 0, so sign(out) = sign(a + b)).
__global__ __launch_bounds__(256) void add_lrelu_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        int64_t n4, float slope, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const float4 u = ld4(a + 4 * t), v = ld4(b + 4 * t);
    float4 o = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    o.x = o.x > 0.f ? o.x : slope * o.x;
    o.y = o.y > 0.f ? o.y : slope * o.y;
    o.z = o.z > 0.f ? o.z : slope * o.z;
    o.w = o.w > 0.f ? o.w : slope * o.w;
    st4(out + 4 * t, o);
}

__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                        int64_t n4, float slope, float* __restrict__ gin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const float4 u = ld4(g + 4 * t), o = ld4(out + 4 * t);
    st4(gin + 4 * t, make_float4(o.x > 0.f ? u.x : slope * u.x, o.y > 0.f ? u.y : slope * u.y,
                                 o.z > 0.f ? u.z : slope * u.z, o.w > 0.f ? u.w : slope * u.w));
}

// gin = mask(a + b; ref, slope): add_lrelu_kernel(slope 1) followed by lrelu_bwd_kernel, the sum kept in registers
__global__ __launch_bounds__(256) void add_mask_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ ref, int64_t n4, float slope,
                                                       float* __restrict__ gin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const float4 u = ld4(a + 4 * t), v = ld4(b + 4 * t), o = ld4(ref + 4 * t);
    const float4 s = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    st4(gin + 4 * t, make_float4(o.x > 0.f ? s.x : slope * s.x, o.y > 0.f ? s.y : slope * s.y,
                                 o.z > 0.f ? s.z : slope * s.z, o.w > 0.f ? s.w : slope * s.w));
}

}  // namespace crf

using namespace crf;

// The two entries of the pooling family refuse everything with CRF_ERR_ARG.
static int check_pool(int64_t rows, int C, int K) {
    CRF_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31), CRF_ERR_ARG, "rows=%lld out of range", (long long)rows);
    CRF_REQUIRE(C > 0 && C % 4 == 0, CRF_ERR_ARG, "channels C=%d must be a positive multiple of 4", C);
    CRF_REQUIRE(K >= 1, CRF_ERR_ARG, "K=%d must be at least 1", K);
    return CRF_OK;
}

extern "C" int crfconv_neighbor_pool_forward(const float* x, const int32_t* idx32, int K, int64_t m_tgt, int C, int reduce,
                                             float* out, int32_t* arg, int32_t* count, crf_stream_t stream) {
    if (int rc = check_pool(m_tgt, C, K)) return rc;
    CRF_REQUIRE(reduce >= POOL_SUM && reduce <= POOL_MIN, CRF_ERR_ARG, "reduce=%d is none of 0 (sum), 1 (mean), 2 (max), 3 (min)", reduce);
    CRF_REQUIRE(x && idx32 && out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(arg || reduce < POOL_MAX, CRF_ERR_ARG, "max and min need arg");
    CRF_REQUIRE(count || reduce != POOL_MEAN, CRF_ERR_ARG, "mean needs count");
    const int64_t n = m_tgt * (C / 4);
    const dim3 grid((unsigned)cdiv(n, 256)), block(256);
    switch (reduce) {
    case POOL_SUM:
        hipLaunchKernelGGL(pool_fwd_kernel<POOL_SUM>, grid, block, 0, as_stream(stream), x, idx32, K, m_tgt, C / 4, out, arg, count);
        break;
    case POOL_MEAN:
        hipLaunchKernelGGL(pool_fwd_kernel<POOL_MEAN>, grid, block, 0, as_stream(stream), x, idx32, K, m_tgt, C / 4, out, arg, count);
        break;
    case POOL_MIN:
        hipLaunchKernelGGL(pool_fwd_kernel<POOL_MIN>, grid, block, 0, as_stream(stream), x, idx32, K, m_tgt, C / 4, out, arg, count);
        break;
    default:
        hipLaunchKernelGGL(maxpool_fwd_kernel<false>, grid, block, 0, as_stream(stream), x, idx32, K, m_tgt, C / 4, out, arg,
                           (const float*)nullptr);
        if (count) {
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(pool_count_kernel, dim3((unsigned)cdiv(m_tgt, 256)), block, 0, as_stream(stream), idx32, K, m_tgt, count);
        }
    }
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// out[i,c] = max_k (a[c] x[idx32[i,k], c] + b[c]),  coef = [a | b | ...] (the [4, C] block of crfconv_bn_coef_from_records).
extern "C" int crfconv_neighbor_maxpool_affine_forward(const float* x, const float* coef, const int32_t* idx32, int K,
                                                       int64_t m_tgt, int C, float* out, int32_t* arg, crf_stream_t stream) {
    if (int rc = check(m_tgt, C)) return rc;
    CRF_REQUIRE(x && coef && idx32 && out && arg && K >= 1, CRF_ERR_ARG, "null pointer / K");
    const int64_t n = m_tgt * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_kernel<true>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), x,
                       idx32, K, m_tgt, C / 4, out, arg, coef);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_neighbor_maxpool_backward(const float* gout, const int32_t* arg,
                                                 const int32_t* rev_ptr, const int32_t* rev_eid, int K,
                                                 int64_t m_src, int C, float* dx, crf_stream_t stream) {
    if (int rc = check(m_src, C)) return rc;
    CRF_REQUIRE(gout && arg && rev_ptr && rev_eid && dx && K >= 1, CRF_ERR_ARG, "null pointer / K");
    const int64_t n = m_src * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream),
                       gout, arg, rev_ptr, rev_eid, K, m_src, C / 4, dx);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_gather_rows(const float* x, const int32_t* idx32, int64_t m_tgt, int C, float* out,
                                   crf_stream_t stream) {
    if (int rc = check(m_tgt, C)) return rc;
    CRF_REQUIRE(x && idx32 && out, CRF_ERR_ARG, "null pointer");
    const int64_t n = m_tgt * (C / 4);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), x,
                       idx32, m_tgt, C / 4, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_neighbor_pool_backward(const float* gout, const int32_t* count, const int32_t* rev_ptr,
                                              const int32_t* rev_eid, int K, int64_t m_src, int C, float* dx, crf_stream_t stream) {
    if (int rc = check_pool(m_src, C, K)) return rc;
    CRF_REQUIRE(gout && rev_ptr && rev_eid && dx, CRF_ERR_ARG, "null pointer");
    const int64_t n = m_src * (C / 4);
    const dim3 grid((unsigned)cdiv(n, 256)), block(256);
    auto kernel = K == 1 ? (count ? pool_bwd_kernel<true, true> : pool_bwd_kernel<true, false>)
                         : (count ? pool_bwd_kernel<false, true> : pool_bwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), gout, count, rev_ptr, rev_eid, K, m_src, C / 4, dx);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_add_lrelu(const float* a, const float* b, int64_t n, float slope, float* out, crf_stream_t stream) {
    CRF_REQUIRE(a && b && out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0 && n % 4 == 0 && n < ((int64_t)1 << 40), CRF_ERR_ARG, "n=%lld must be a positive multiple of 4", (long long)n);
    CRF_REQUIRE(slope > 0.f, CRF_ERR_ARG, "slope must be positive");
    hipLaunchKernelGGL(crf::add_lrelu_kernel, dim3((unsigned)crf::cdiv(n / 4, 256)), dim3(256), 0, crf::as_stream(stream), a, b,
                       n / 4, slope, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_add_lrelu_backward(const float* gout, const float* out, int64_t n, float slope, float* gin,
                                          crf_stream_t stream) {
    CRF_REQUIRE(gout && out && gin, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0 && n % 4 == 0 && n < ((int64_t)1 << 40), CRF_ERR_ARG, "n=%lld must be a positive multiple of 4", (long long)n);
    hipLaunchKernelGGL(crf::lrelu_bwd_kernel, dim3((unsigned)crf::cdiv(n / 4, 256)), dim3(256), 0, crf::as_stream(stream), gout,
                       out, n / 4, slope, gin);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_add_mask(const float* a, const float* b, const float* ref, int64_t n, float slope, float* gin,
                                crf_stream_t stream) {
    CRF_REQUIRE(a && b && ref && gin, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0 && n % 4 == 0 && n < ((int64_t)1 << 40), CRF_ERR_ARG, "n=%lld must be a positive multiple of 4", (long long)n);
    hipLaunchKernelGGL(crf::add_mask_kernel, dim3((unsigned)crf::cdiv(n / 4, 256)), dim3(256), 0, crf::as_stream(stream), a, b, ref,
                       n / 4, slope, gin);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
