// CRF mean-field, gfx950: the backward of the generic path, one step per call -- any K <= 64, any k0, entries < 0 = no neighbour
// (the padded variable-degree tables of the sparse operators).  A step's backward is two launches (edge half, scatter half), the
// similarity's two more; ops/crf.py chains them.  The fast shapes (K in {16, 32}, k0 = 1) train through crf_bwd.hip instead; these
// kernels give the same results for them.  The edge half of a step (bwd_edge_kernel, crfconv_meanfield_bwd_edge) is in crf.hip, whose
// header says why.  Thread mapping and layout: the header of crf.hip too.
#include "crf_common.hpp"

namespace crf {

// ====================================================================== backward, scatter half

template <int H>
__global__ __launch_bounds__(BLOCK) void bwd_scatter_kernel(const float* __restrict__ gm,
                                                            const float* __restrict__ s,
                                                            const int32_t* __restrict__ rev_ptr,
                                                            const int32_t* __restrict__ rev_eid,
                                                            int K, int kshift,
                                                            const float* __restrict__ add,
                                                            float* __restrict__ Gprev,
                                                            int64_t m_src) {
    constexpr int L = Scat<H>::L, EP = Scat<H>::EP;
    const int lane = threadIdx.x & 63;
    const int q = lane % L, el = (lane / L) % EP;
    int64_t row = (int64_t)xcd_block_id() * Scat<H>::RPB + (threadIdx.x >> 6) * Scat<H>::RPW + lane / (L * EP);
    const bool valid = row < m_src;
    if (!valid) row = m_src - 1;                    // keep every lane in the shuffles below
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int beg = rev_ptr[row], end = valid ? rev_ptr[row + 1] : beg;
#pragma unroll 2
    for (int p = beg + el; p < end; p += EP) {
        const int e = rev_eid[p];
        const int i = kshift >= 0 ? (e >> kshift) : (e / K);
        acc = fma4(s[e], ld4(gm + (int64_t)i * H + 4 * q), acc);
    }
    acc = fold_edge_lanes<H>(acc);
    if (valid && el == 0) {
        if (add) {
            const float4 a0 = ld4(add + row * H + 4 * q);
            acc = make_float4(acc.x + a0.x, acc.y + a0.y, acc.z + a0.z, acc.w + a0.w);
        }
        st4(Gprev + row * H + 4 * q, acc);
    }
}

// ====================================================================== softmax / distance backward
template <int H>
__global__ __launch_bounds__(BLOCK) void sim_bwd_kernel(const float* __restrict__ ds,
                                                        const float* __restrict__ s,
                                                        const float* __restrict__ y,
                                                        const int32_t* __restrict__ idx, int K,
                                                        int k0, float* __restrict__ w,
                                                        float* __restrict__ dy_self, int64_t m) {
    constexpr int L = Geo<H>::L;
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);
    const int32_t* irow = idx + r * K;
    const float* srow = s + r * K;
    const float* dsrow = ds + r * K;
    float* wrow = w + r * K;
    float dotv = 0.f;
    for (int k = k0; k < K; ++k) dotv = fmaf(srow[k], dsrow[k], dotv);
    const float4 yi = ld4(y + r * H + 4 * q);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k = k0; k < K; ++k) {
        // d loss / d logit_k = s_k (ds_k - dot);  logit = -dist  =>  d/d dist = -that;  w = 2 * d/d dist
        const float wk = -2.0f * srow[k] * (dsrow[k] - dotv);      // 0 on missing entries (s == 0)
        const int j = irow[k];
        acc = fma4(wk, sub4(yi, ld4(y + (int64_t)(j >= 0 ? j : 0) * H + 4 * q)), acc);
        if (valid && q == (k % L)) wrow[k] = wk;
    }
    if (valid && q == 0)
        for (int k = 0; k < k0; ++k) wrow[k] = 0.f;
    if (valid) st4(dy_self + r * H + 4 * q, acc);
}

// dy[j] = dy_self[j] + sum_{e in rev(j)} w[e] (y_j - y_{e/K})       (w is 0 on columns < k0)
template <int H>
__global__ __launch_bounds__(BLOCK) void sim_bwd_scatter_kernel(const float* __restrict__ w,
                                                                const float* __restrict__ y,
                                                                const float* __restrict__ dy_self,
                                                                const int32_t* __restrict__ rev_ptr,
                                                                const int32_t* __restrict__ rev_eid,
                                                                int K, int kshift,
                                                                float* __restrict__ dy,
                                                                int64_t m_src) {
    constexpr int L = Scat<H>::L, EP = Scat<H>::EP;
    const int lane = threadIdx.x & 63;
    const int q = lane % L, el = (lane / L) % EP;
    int64_t row = (int64_t)xcd_block_id() * Scat<H>::RPB + (threadIdx.x >> 6) * Scat<H>::RPW + lane / (L * EP);
    const bool valid = row < m_src;
    if (!valid) row = m_src - 1;
    const float4 yj = ld4(y + row * H + 4 * q);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int beg = rev_ptr[row], end = valid ? rev_ptr[row + 1] : beg;
    constexpr int UB = SCAT_UB;                     // edge ids, then weights + rows, in batches (see bwd_chain_kernel)
    for (int p0 = beg + el; p0 < end; p0 += EP * UB) {
        int e[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int p = p0 + u * EP;
            e[u] = p < end ? rev_eid[p] : -1;
        }
        float we[UB];
        float4 g[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int ee = e[u] >= 0 ? e[u] : 0;
            const int i = kshift >= 0 ? (ee >> kshift) : (ee / K);
            we[u] = e[u] >= 0 ? w[ee] : 0.f;
            g[u] = ld4(y + (int64_t)i * H + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) acc = fma4(we[u], sub4(yj, g[u]), acc);
    }
    acc = fold_edge_lanes<H>(acc);
    if (valid && el == 0) {
        const float4 a0 = ld4(dy_self + row * H + 4 * q);
        st4(dy + row * H + 4 * q, make_float4(acc.x + a0.x, acc.y + a0.y, acc.z + a0.z, acc.w + a0.w));
    }
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_meanfield_bwd_scatter(const float* gm, const float* s, const int32_t* rev_ptr,
                                             const int32_t* rev_eid, int K, int k0, int64_t m_src,
                                             int H, const float* add, float* Gprev,
                                             crf_stream_t stream) {
    if (int rc = check_common(m_src, H, K, k0)) return rc;
    CRF_REQUIRE(gm && s && rev_ptr && rev_eid && Gprev, CRF_ERR_ARG, "null pointer");
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) {
        constexpr int HH = decltype(HC)::value;
        hipLaunchKernelGGL(bwd_scatter_kernel<HH>, dim3((unsigned)cdiv(m_src, Scat<HH>::RPB)), dim3(BLOCK), 0, as_stream(stream), gm, s,
                           rev_ptr, rev_eid, K, kshift_of(K), add, Gprev, m_src);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_similarity_bwd(const float* ds, const float* s, const float* y,
                                      const int32_t* idx32, int K, int k0, int64_t m, int H, float* w,
                                      float* dy_self, crf_stream_t stream) {
    if (int rc = check_common(m, H, K, k0)) return rc;
    CRF_REQUIRE(ds && s && y && idx32 && w && dy_self, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(w != ds, CRF_ERR_ARG, "w must not alias ds");
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) {
        constexpr int HH = decltype(HC)::value;
        hipLaunchKernelGGL(sim_bwd_kernel<HH>, dim3((unsigned)cdiv(m, Geo<HH>::PPB)), dim3(BLOCK), 0, as_stream(stream), ds, s, y, idx32,
                           K, k0, w, dy_self, m);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_similarity_bwd_scatter(const float* w, const float* y, const float* dy_self,
                                              const int32_t* rev_ptr, const int32_t* rev_eid, int K,
                                              int k0, int64_t m_src, int H, float* dy,
                                              crf_stream_t stream) {
    if (int rc = check_common(m_src, H, K, k0)) return rc;
    CRF_REQUIRE(w && y && dy_self && rev_ptr && rev_eid && dy, CRF_ERR_ARG, "null pointer");
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) {
        constexpr int HH = decltype(HC)::value;
        hipLaunchKernelGGL(sim_bwd_scatter_kernel<HH>, dim3((unsigned)cdiv(m_src, Scat<HH>::RPB)), dim3(BLOCK), 0, as_stream(stream), w, y,
                           dy_self, rev_ptr, rev_eid, K, kshift_of(K), dy, m_src);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
