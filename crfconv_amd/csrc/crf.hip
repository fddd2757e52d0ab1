// CRF mean-field kernels for gfx950: the per-step forward for H <= 64 (similarity, then one launch per step).  The per-step
// backward of the generic path is crf_step_bwd.hip, the backward of the fast shapes crf_bwd.hip, the one-launch forward
// crf_block.hip, H = 128 / 256 crf_wide.hip.
//
// One kernel of the per-step backward stays here with its entry: bwd_edge_kernel.  It and step_kernel are the two callers of
// load_matrix<H> with a loop (H = 32, 64), one with transpose = true, one with false; with each alone in its unit both compile
// to other instruction orders at H = 32 and 64 (same word counts and registers), together to the code they always had.
//
// Thread mapping (all kernels of these units but the wide ones): a point's H channels are spread over L = H/4 adjacent lanes,
// one float4 (16-byte load) per lane, so a 64-lane wavefront carries 64/L points and a
// neighbour row is fetched by L lanes as one contiguous 4H-byte segment.  Per-point reductions
// (squared distance, dot products) are xor-shuffles over the L lanes; the H x H products use
// shuffles for the vector and LDS (float4 rows) for the matrix.
//
// Layout: every per-edge array (s, ds, w) is [m, K] with the SAME column index as the neighbour
// table (columns < k0 hold 0), i.e. it is addressed by the edge id e = i*K + k.  With K = 16 a
// row of indices and a row of weights are each one aligned 64-byte segment: the fast kernels
// (K = 16 / 32, k0 = 1) pull them with dwordx4 loads and keep them in registers, so all K-1
// neighbour gathers of a point are in flight together.
//
// Reference semantics: models/continuous_crf_conv_big.py:49-54 (similarity), :63-72 (loop).
#include "crf_common.hpp"

#ifndef CRF_GATHER_SRD
#define CRF_GATHER_SRD 1      // neighbour rows through a buffer resource with 32-bit byte offsets (0: generic 64-bit pointers, the A/B baseline)
#endif

#ifndef SIM_WAVES_
#define SIM_WAVES_ 4          // wavefronts per SIMD the level-0 first kernel is compiled for (A/B: 5 = the whole 4 x 40960 grid co-resident)
#endif

namespace crf {


// ====================================================================== fast forward kernels
// (K in {16, 32}, k0 == 1).  FIRST = similarity + z Q + first step fused: the index row is read
// once, s never round-trips through memory before its first use.
template <int H, int K, bool WITH_STEP, bool U16>
__global__ __launch_bounds__(BLOCK, (H == 8 && K == 16) ? SIM_WAVES_ : 1) void sim_step_fast_kernel(const float* __restrict__ y,
                                                              const float* __restrict__ z,
                                                              const int32_t* __restrict__ idx,
                                                              const uint16_t* __restrict__ idx16, int n_tgt, int n_src,
                                                              const float* __restrict__ Q,
                                                              const float* __restrict__ P,
                                                              float* __restrict__ s,
                                                              float* __restrict__ x1, int64_t m) {
    constexpr int L = Geo<H>::L;
    __shared__ float4 sQ[WITH_STEP ? MatStage<H>::F4 : 1];
    __shared__ float4 sP[WITH_STEP ? MatStage<H>::F4 : 1];
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);

    // issue order = arrival order: the index row first (the gathers wait for nothing else), then the own rows and the
    // matrices, which are only needed behind the gathers
#if CRF_GATHER_SRD
    int off[K];                                   // byte offsets of the neighbour rows: buffer loads, 32-bit address arithmetic
    load_index_offsets_t<K, U16, H>(idx, idx16, r, n_tgt, n_src, q, off);
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(y, (int)(m * H * 4));
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rz = make_rsrc(z, (int)(m * H * 4));
#else
    int j[K];
    load_index_row_t<K, U16>(idx, idx16, r, n_tgt, n_src, j);
#endif
    const float4 yi = ld4(y + r * H + 4 * q);
    [[maybe_unused]] float4 zi = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] MatStage<H> mq, mp;
    if constexpr (WITH_STEP) {
        zi = ld4(z + r * H + 4 * q);
        mq.fetch(Q, false);
        mp.fetch(P, false);
    }
    float4 nb[K];
#pragma unroll
#if CRF_GATHER_SRD
    for (int k = 1; k < K; ++k) nb[k] = ld4_buf(ry, off[k]);
#else
    for (int k = 1; k < K; ++k) nb[k] = ld4(y + (int64_t)j[k] * H + 4 * q);
#endif
    float d[K];
    float dmin = 3.4e38f;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const float4 df = sub4(yi, nb[k]);
        d[k] = group_sum<L>(dot4(df, df));
        dmin = fminf(dmin, d[k]);
    }
    if constexpr (WITH_STEP) {   // issue the z-row gathers before the exp chain
#pragma unroll
#if CRF_GATHER_SRD
        for (int k = 1; k < K; ++k) nb[k] = ld4_buf(rz, off[k]);
#else
        for (int k = 1; k < K; ++k) nb[k] = ld4(z + (int64_t)j[k] * H + 4 * q);
#endif
        mq.park(sQ);
        mp.park(sP);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        d[k] = __expf(dmin - d[k]);        // v_exp_f32 path: ~1e-7 relative, far inside the 1e-4 budget
        den += d[k];
    }
    const float inv = 1.0f / den;
    d[0] = 0.f;
#pragma unroll
    for (int k = 1; k < K; ++k) d[k] *= inv;
    if (s != nullptr) store_rows_coalesced<H, K>(d, s, lane, q, m);       // NULL: inference with T <= 1, nobody re-reads s

    if constexpr (WITH_STEP) {
        float4 msg = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 1; k < K; ++k) msg = fma4(d[k], nb[k], msg);
        __syncthreads();
        const float4 zqi = matvec_acc<H>(zi, sQ, lane, q, make_float4(0.f, 0.f, 0.f, 0.f));
        const float4 o = matvec_acc<H>(msg, sP, lane, q, zqi);
        if (valid) st4(x1 + r * H + 4 * q, o);
    }
}

template <int H, int K, bool U16>
__global__ __launch_bounds__(BLOCK) void step_fast_kernel(const float* __restrict__ xin,
                                                          const float* __restrict__ z,
                                                          const float* __restrict__ s,
                                                          const int32_t* __restrict__ idx,
                                                          const uint16_t* __restrict__ idx16, int n_tgt, int n_src,
                                                          const float* __restrict__ Q,
                                                          const float* __restrict__ P,
                                                          float* __restrict__ xout, int64_t m) {
    __shared__ float4 sP[MatStage<H>::F4];
    __shared__ float4 sQ[MatStage<H>::F4];
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);
    float w[K];
#if CRF_GATHER_SRD
    int off[K];
    load_index_offsets_t<K, U16, H>(idx, idx16, r, n_tgt, n_src, q, off);  // first: the gathers wait for this row only
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(xin, (int)(m * H * 4));
#define CRF_GATHER_X(k) ld4_buf(rx, off[k])
#else
    int j[K];
    load_index_row_t<K, U16>(idx, idx16, r, n_tgt, n_src, j);              // first: the gathers wait for this row only
#define CRF_GATHER_X(k) ld4(xin + (int64_t)j[k] * H + 4 * q)
#endif
    load_row<K, float4>(s + r * K, w);
    const float4 zi = ld4(z + r * H + 4 * q);
    MatStage<H> mp, mq;
    mp.fetch(P, false);
    mq.fetch(Q, false);
    // gathers in two batches of K/2 (fewer live registers: 8 waves/SIMD at H = 8, K = 16; measured 0.2-0.3 us faster)
    float4 msg = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        float4 nb[K / 2];
#pragma unroll
        for (int k = 1; k < K / 2; ++k) nb[k] = CRF_GATHER_X(k);
        mp.park(sP);
        mq.park(sQ);
#pragma unroll
        for (int k = 1; k < K / 2; ++k) msg = fma4(w[k], nb[k], msg);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) nb[k] = CRF_GATHER_X(K / 2 + k);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) msg = fma4(w[K / 2 + k], nb[k], msg);
    }
    __syncthreads();
    // z Q recomputed from z (same bytes as reading a stored z Q, and nothing extra to write)
    const float4 zqi = matvec_acc<H>(zi, sQ, lane, q, make_float4(0.f, 0.f, 0.f, 0.f));
    const float4 o = matvec_acc<H>(msg, sP, lane, q, zqi);
    if (valid) st4(xout + r * H + 4 * q, o);
#undef CRF_GATHER_X
}

// (The one-launch forward -- all T steps behind grid barriers, mf_fused_kernel -- and the LDS-window kernels of rounds 1-3 were
// measured slower than the per-step launches (39-40 us against 25 us; 43.0 against 39.5 us: DESIGN.md 5c, profiles/r2a_*) and
// were removed in round 4; `git log -- crfconv_amd/csrc/crf.hip` has them.)

// ====================================================================== generic forward kernels
// any K <= 64, any k0: distances recomputed in a second sweep (rows are L1/L2 hot by then).
template <int H>
__global__ __launch_bounds__(BLOCK) void sim_kernel(const float* __restrict__ y,
                                                    const int32_t* __restrict__ idx, int K, int k0,
                                                    float* __restrict__ s, int64_t m) {
    constexpr int L = Geo<H>::L;
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);
    const float4 yi = ld4(y + r * H + 4 * q);
    const int32_t* irow = idx + r * K;
    float* srow = s + r * K;

    // entries < 0 mark "no neighbour" (padded variable-degree tables of the sparse operators)
    auto dist_to = [&](int k, bool& have) {
        const int j = irow[k];
        have = j >= 0;
        const float4 df = sub4(yi, ld4(y + (int64_t)(have ? j : 0) * H + 4 * q));
        return group_sum<L>(dot4(df, df));
    };
    float dmin = 3.4e38f;
    for (int k = k0; k < K; ++k) {
        bool have;
        const float dk = dist_to(k, have);
        if (have) dmin = fminf(dmin, dk);
    }
    float den = 0.f;
    for (int k = k0; k < K; ++k) {
        bool have;
        const float dk = dist_to(k, have);
        const float e = have ? expf(dmin - dk) : 0.f;
        den += e;
        if (valid && q == 0) srow[k] = e;
    }
    const float inv = den > 0.f ? 1.0f / den : 0.f;      // isolated point: no message
    if (valid && q == 0) {  // same lane re-reads what it wrote
        for (int k = 0; k < k0; ++k) srow[k] = 0.f;
        for (int k = k0; k < K; ++k) srow[k] *= inv;
    }
}

template <int H>
__global__ __launch_bounds__(BLOCK) void step_kernel(const float* __restrict__ xin,
                                                     const float* __restrict__ z,
                                                     const float* __restrict__ s,
                                                     const int32_t* __restrict__ idx, int K, int k0,
                                                     const float* __restrict__ Q,
                                                     const float* __restrict__ P,
                                                     float* __restrict__ xout, int64_t m) {
    constexpr int L = Geo<H>::L;
    __shared__ float4 sP[H * L];
    __shared__ float4 sQ[H * L];
    load_matrix<H>(sP, P, false);
    load_matrix<H>(sQ, Q, false);
    __syncthreads();
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);
    const int32_t* irow = idx + r * K;
    const float* srow = s + r * K;
    float4 msg = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k = k0; k < K; ++k) {
        const int j = irow[k];
        if (j >= 0) msg = fma4(srow[k], ld4(xin + (int64_t)j * H + 4 * q), msg);
    }
    const float4 zqi = matvec_acc<H>(ld4(z + r * H + 4 * q), sQ, lane, q, make_float4(0.f, 0.f, 0.f, 0.f));
    const float4 o = matvec_acc<H>(msg, sP, lane, q, zqi);
    if (valid) st4(xout + r * H + 4 * q, o);
}

// ====================================================================== backward, edge half (its scatter half: crf_step_bwd.hip;
// why here: the file header)
// gm = G P^T ; ds[i,k] (+)= <gm_i, xprev_j> ; mt_i = sum_k s_ik xprev_j.
template <int H>
__global__ __launch_bounds__(BLOCK) void bwd_edge_kernel(const float* __restrict__ G,
                                                         const float* __restrict__ xprev,
                                                         const float* __restrict__ s,
                                                         const int32_t* __restrict__ idx, int K,
                                                         int k0, const float* __restrict__ P,
                                                         float* __restrict__ gm,
                                                         float* __restrict__ ds,
                                                         float* __restrict__ mt, int accumulate,
                                                         int64_t m) {
    constexpr int L = Geo<H>::L;
    __shared__ float4 sPT[H * L];
    load_matrix<H>(sPT, P, true);
    __syncthreads();
    int lane, q;
    bool valid;
    const int64_t r = my_point<H>(m, lane, q, valid);
    const float4 g = ld4(G + r * H + 4 * q);
    const float4 gmi = matvec_acc<H>(g, sPT, lane, q, make_float4(0.f, 0.f, 0.f, 0.f));
    if (valid) st4(gm + r * H + 4 * q, gmi);
    float4 msg = make_float4(0.f, 0.f, 0.f, 0.f);
    const int32_t* irow = idx + r * K;
    const float* srow = s + r * K;
    float* dsrow = ds + r * K;
#pragma unroll 4
    for (int k = k0; k < K; ++k) {
        const int j = irow[k];
        const bool have = j >= 0;
        float4 xj = ld4(xprev + (int64_t)(have ? j : 0) * H + 4 * q);
        if (!have) xj = make_float4(0.f, 0.f, 0.f, 0.f);
        msg = fma4(srow[k], xj, msg);
        const float dotv = group_sum<L>(dot4(gmi, xj));
        if (valid && q == (k % L)) dsrow[k] = accumulate ? dsrow[k] + dotv : dotv;
    }
    if (valid && q == 0 && !accumulate)
        for (int k = 0; k < k0; ++k) dsrow[k] = 0.f;
    if (mt != nullptr && valid) st4(mt + r * H + 4 * q, msg);
}

}  // namespace crf

using namespace crf;

static int meanfield_forward_impl(const float* z, const float* y, const int32_t* idx32, const uint16_t* idx16,
                                  int n_tgt, int n_src, int K, int k0, int64_t m, int H, const float* Q,
                                  const float* P, int T, float* s, float* xs, crf_stream_t stream) {
    if (int rc = check_common(m, H, K, k0)) return rc;
    CRF_REQUIRE(z && y && idx32 && Q && P && (xs || T == 0), CRF_ERR_ARG, "null pointer");
    // (the fast kernels address neighbour rows by 32-bit byte offsets: tables of 2 GiB and more take the generic kernels)
    const bool fast = fast_shape(K, k0) && m * H * 4 < ((int64_t)1 << 31);
    // s may be NULL when nothing reads it back: a single fused step (T == 1) on the fast path, no backward pass
    CRF_REQUIRE(s || (T == 1 && fast), CRF_ERR_ARG,
                "s == NULL needs T == 1 on the fused first-step kernel (K in {16, 32}, k0 == 1)");
    CRF_REQUIRE(T >= 0, CRF_ERR_ARG, "T=%d < 0", T);
    hipStream_t st = as_stream(stream);
    // the fast kernels' template arguments: K, the fused first step, the index layout (uint16 local ids / int32 global rows)
    auto launches = [&](auto HC) -> int {
        constexpr int HH = decltype(HC)::value;
        const dim3 grid((unsigned)cdiv(m, Geo<HH>::PPB)), blk(BLOCK);
        if (fast) {
            dispatch_width(Widths<16, 32>{}, K, [&](auto KC) {
                dispatch_flag(T > 0, [&](auto WS) {
                    dispatch_flag(idx16 != nullptr, [&](auto U16) {
                        hipLaunchKernelGGL((sim_step_fast_kernel<HH, decltype(KC)::value, decltype(WS)::value, decltype(U16)::value>), grid, blk,
                                           0, st, y, z, idx32, idx16, n_tgt, n_src, Q, P, s, T > 0 ? xs : nullptr, m);
                    });
                });
            });
        } else {
            hipLaunchKernelGGL(sim_kernel<HH>, grid, blk, 0, st, y, idx32, K, k0, s, m);
        }
        CRF_LAUNCH_CHECK();
        for (int t = fast ? 1 : 0; t < T; ++t) {
            const float* xin = t == 0 ? z : xs + (int64_t)(t - 1) * m * H;
            float* xout = xs + (int64_t)t * m * H;
            if (fast) {
                dispatch_width(Widths<16, 32>{}, K, [&](auto KC) {
                    dispatch_flag(idx16 != nullptr, [&](auto U16) {
                        hipLaunchKernelGGL((step_fast_kernel<HH, decltype(KC)::value, decltype(U16)::value>), grid, blk, 0, st, xin, z, s,
                                           idx32, idx16, n_tgt, n_src, Q, P, xout, m);
                    });
                });
            } else {
                hipLaunchKernelGGL(step_kernel<HH>, grid, blk, 0, st, xin, z, s, idx32, K, k0, Q, P, xout, m);
            }
            CRF_LAUNCH_CHECK();
        }
        return CRF_OK;
    };
    int rc = CRF_OK;
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) { rc = launches(HC); });
    return rc;
}

extern "C" int crfconv_meanfield_forward(const float* z, const float* y, const int32_t* idx32, int K,
                                         int k0, int64_t m, int H, const float* Q, const float* P,
                                         int T, float* s, float* xs, crf_stream_t stream) {
    return meanfield_forward_impl(z, y, idx32, nullptr, 1, 1, K, k0, m, H, Q, P, T, s, xs, stream);
}

extern "C" int crfconv_meanfield_forward_u16(const float* z, const float* y, const int32_t* idx32,
                                             const uint16_t* idx16, int n_tgt, int n_src, int K, int k0,
                                             int64_t m, int H, const float* Q, const float* P, int T, float* s,
                                             float* xs, crf_stream_t stream) {
    if (int rc = check_u16(idx16, n_tgt, n_src, m)) return rc;
    return meanfield_forward_impl(z, y, idx32, idx16, n_tgt, n_src, K, k0, m, H, Q, P, T, s, xs, stream);
}

// One step with GIVEN edge weights: xout = z Q + (sum_k s_ik xin_{j(i,k)}) P  (generic kernel: any K <= 64, k0,
// entries < 0 = no neighbour).  The discrete CRF layer (models/discrete_crf_conv.py:57-61) runs on this.
extern "C" int crfconv_meanfield_step(const float* xin, const float* z, const float* s, const int32_t* idx32, int K,
                                      int k0, int64_t m, int H, const float* Q, const float* P, float* xout,
                                      crf_stream_t stream) {
    if (int rc = check_common(m, H, K, k0)) return rc;
    CRF_REQUIRE(xin && z && s && idx32 && Q && P && xout, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(xin != xout, CRF_ERR_ARG, "xout must not alias xin");
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) {
        constexpr int HH = decltype(HC)::value;
        hipLaunchKernelGGL(step_kernel<HH>, dim3((unsigned)cdiv(m, Geo<HH>::PPB)), dim3(BLOCK), 0, as_stream(stream), xin, z, s, idx32, K,
                           k0, Q, P, xout, m);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_meanfield_bwd_edge(const float* G, const float* xprev, const float* s,
                                          const int32_t* idx32, int K, int k0, int64_t m, int H,
                                          const float* P, float* gm, float* ds, float* mt,
                                          int accumulate, crf_stream_t stream) {
    if (int rc = check_common(m, H, K, k0)) return rc;
    CRF_REQUIRE(G && xprev && s && idx32 && P && gm && ds, CRF_ERR_ARG, "null pointer");
    dispatch_width(CRF_WIDTHS, H, [&](auto HC) {
        constexpr int HH = decltype(HC)::value;
        hipLaunchKernelGGL(bwd_edge_kernel<HH>, dim3((unsigned)cdiv(m, Geo<HH>::PPB)), dim3(BLOCK), 0, as_stream(stream), G, xprev, s,
                           idx32, K, k0, P, gm, ds, mt, accumulate, m);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
