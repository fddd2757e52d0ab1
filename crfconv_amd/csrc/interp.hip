// kNN interpolation (torch_geometric.nn.knn_interpolate), gfx950: the inverse-squared-distance blend of a table's source rows and
// its transpose, the only operator on the sparse networks' forward path that ran as framework kernels (a gather of positions, a
// subtract, a square, a sum, a clamp, a reciprocal, a gather of features, two index_add_ and a divide; float atomics behind them).
//
// Table idx32 [n_y, K]: global rows of x; an entry < 0 or >= n_x means "no neighbour" (the segmented kNN pads with -1).
//
//   interp_fwd   per target row i, slots s = 0 .. K-1 IN THAT ORDER:
//                    d = pos_y[i] - pos_x[j],  w = 1 / max(dx dx + dy dy + dz dz, 1e-16f),  den += w,  num[c] += w x[j, c]
//                out[i, c] = num[c] / den;  coef[i, s] = w / den when asked for, 0 in a skipped slot.
//                A row WITHOUT any valid slot gives a zero out row and zero coef (the composition this replaces divided 0 by 0
//                there and returned NaN).
//   interp_bwd   per source row j:  out[j, c] = sum_e coef[e] g[e / K, c]  over e in rev_eid[rev_ptr[j] .. rev_ptr[j + 1]) in the stored
//                (ascending) order; an empty list gives a zero row.  No atomics: the result is the same bits in every run.
//
// Thread mapping, both directions: a row is cut into pieces of VW channels (VW = 4: float4 loads and stores, taken when C % 4 == 0 and
// every row is 16-byte aligned; VW = 1 otherwise); `lanes` lanes share a row, 256 / lanes rows a workgroup (rows wider than 256 lanes:
// one row per workgroup, a lane walks on).  Every lane of a row forms the row's weights itself -- K index loads and K 12-byte position
// loads, the same addresses across the row's lanes, which hit in cache -- so nothing crosses lanes and no row needs a whole wavefront.
// coef is written once per row.
// Pieces per lane, picked by measurement (131072 targets from 32768 sources, K = 3; kernel trace, profiles/r19_interpolate.md): in the
// FORWARD a lane owns PP = 4 pieces of its row, `lanes` pieces apart, when the row's pieces divide by four -- the weights are then paid
// once per 16 channels: 16.7 us against 22.0 at C = 64, 103 against 150 at C = 512.  The TRANSPOSE keeps one piece per lane: with four
// it has a quarter of the wavefronts (two per SIMD at C = 64) for the same lists and ran 23 us against 20, 122 against 110.
#include "common.hpp"

namespace crf {

constexpr int IP_BLOCK = 256;

template <int VW>
struct IpVec {
    float v[VW];
    __device__ __forceinline__ void load(const float* __restrict__ p) {
        if constexpr (VW == 4) { const float4 t = ld4(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
        else v[0] = p[0];
    }
    __device__ __forceinline__ void store(float* __restrict__ p) const {
        if constexpr (VW == 4) st4(p, make_float4(v[0], v[1], v[2], v[3]));
        else p[0] = v[0];
    }
};

// w of slot s of row i (0 and j = 0 in a skipped slot); the one place the weight is formed, so out and coef agree bit for bit
__device__ __forceinline__ float ip_weight(const float* __restrict__ pos_x, float yx, float yy, float yz, int jraw, int n_x, int& j) {
    const bool ok = (unsigned)jraw < (unsigned)n_x;
    j = ok ? jraw : 0;                                   // the loads below stay in range and unconditional
    const float* p = pos_x + 3 * (int64_t)j;
    const float dx = yx - p[0], dy = yy - p[1], dz = yz - p[2];
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    return ok ? 1.0f / fmaxf(d2, 1e-16f) : 0.f;
}

// KF: the table's K when it is a compile-time constant (the weights are formed once per lane and kept, every slot's index, position
// and row loads are in flight together), 0 = any K (the weights are formed slot by slot).
template <int VW, int PP, int KF>
__global__ __launch_bounds__(IP_BLOCK) void interp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pos_x,
                                                              const float* __restrict__ pos_y, const int32_t* __restrict__ idx,
                                                              int K, int64_t n_y, int n_x, int C, int lanes, float* __restrict__ coef,
                                                              float* __restrict__ out) {
    const int CW = C / VW;                               // pieces per row
    const int r = (int)threadIdx.x / lanes, q0 = (int)threadIdx.x - r * lanes, rows = IP_BLOCK / lanes;
    const int64_t i = (int64_t)blockIdx.x * rows + r;
    if (r >= rows || i >= n_y) return;
    const float yx = pos_y[3 * i], yy = pos_y[3 * i + 1], yz = pos_y[3 * i + 2];
    const int32_t* row = idx + i * K;
    if constexpr (KF > 0) {
        int j[KF];
        float w[KF], den = 0.f;
#pragma unroll
        for (int s = 0; s < KF; ++s) w[s] = ip_weight(pos_x, yx, yy, yz, row[s], n_x, j[s]);
#pragma unroll
        for (int s = 0; s < KF; ++s) den += w[s];        // (a skipped slot adds 0)
        for (int q = q0; q < CW; q += lanes * PP) {
            IpVec<VW> xj[KF][PP], acc[PP];
#pragma unroll
            for (int s = 0; s < KF; ++s) {
#pragma unroll
                for (int u = 0; u < PP; ++u) xj[s][u].load(x + (int64_t)j[s] * C + VW * (q + u * lanes));
            }
#pragma unroll
            for (int u = 0; u < PP; ++u) {
#pragma unroll
                for (int c = 0; c < VW; ++c) {
                    float a = 0.f;                       // (a skipped slot adds 0 * 0, never 0 * x: x may be non-finite)
#pragma unroll
                    for (int s = 0; s < KF; ++s) a = fmaf(w[s], w[s] > 0.f ? xj[s][u].v[c] : 0.f, a);
                    acc[u].v[c] = den > 0.f ? a / den : 0.f;
                }
                acc[u].store(out + i * C + VW * (q + u * lanes));
            }
        }
        if (coef != nullptr && q0 == 0) {
#pragma unroll
            for (int s = 0; s < KF; ++s) coef[i * KF + s] = den > 0.f ? w[s] / den : 0.f;
        }
    } else {
        float den = 0.f;
        for (int q = q0; q < CW; q += lanes * PP) {
            IpVec<VW> acc[PP];
#pragma unroll
            for (int u = 0; u < PP; ++u) {
#pragma unroll
                for (int c = 0; c < VW; ++c) acc[u].v[c] = 0.f;
            }
            den = 0.f;
            for (int s = 0; s < K; ++s) {
                int j;
                const float w = ip_weight(pos_x, yx, yy, yz, row[s], n_x, j);
                IpVec<VW> xj[PP];
#pragma unroll
                for (int u = 0; u < PP; ++u) xj[u].load(x + (int64_t)j * C + VW * (q + u * lanes));
                den += w;
#pragma unroll
                for (int u = 0; u < PP; ++u) {
#pragma unroll
                    for (int c = 0; c < VW; ++c) acc[u].v[c] = fmaf(w, w > 0.f ? xj[u].v[c] : 0.f, acc[u].v[c]);
                }
            }
#pragma unroll
            for (int u = 0; u < PP; ++u) {
#pragma unroll
                for (int c = 0; c < VW; ++c) acc[u].v[c] = den > 0.f ? acc[u].v[c] / den : 0.f;
                acc[u].store(out + i * C + VW * (q + u * lanes));
            }
        }
        if (coef != nullptr) {
            for (int s = q0; s < K; s += lanes) {        // slot s by lane s of the row (mod its lanes), from the same arithmetic
                int j;
                const float w = ip_weight(pos_x, yx, yy, yz, row[s], n_x, j);
                coef[i * K + s] = den > 0.f ? w / den : 0.f;
            }
        }
    }
}

template <int VW>
__global__ __launch_bounds__(IP_BLOCK) void interp_bwd_kernel(const float* __restrict__ g, const float* __restrict__ coef,
                                                              const int32_t* __restrict__ rev_ptr, const int32_t* __restrict__ rev_eid,
                                                              int K, int64_t n_x, int C, int lanes, float* __restrict__ out) {
    const int CW = C / VW;
    const int r = (int)threadIdx.x / lanes, q0 = (int)threadIdx.x - r * lanes, rows = IP_BLOCK / lanes;
    const int64_t j = (int64_t)blockIdx.x * rows + r;
    if (r >= rows || j >= n_x) return;
    const int beg = rev_ptr[j], end = rev_ptr[j + 1];
    const unsigned uK = (unsigned)K;
    for (int q = q0; q < CW; q += lanes) {
        IpVec<VW> acc;
#pragma unroll
        for (int c = 0; c < VW; ++c) acc.v[c] = 0.f;
        int p = beg;
        for (; p + 4 <= end; p += 4) {                   // four edges' coefficient and row loads in flight, added in list order
            float w[4];
            IpVec<VW> gr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned e = (unsigned)rev_eid[p + u];
                w[u] = coef[e];
                gr[u].load(g + (int64_t)(e / uK) * C + VW * q);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int c = 0; c < VW; ++c) acc.v[c] = fmaf(w[u], gr[u].v[c], acc.v[c]);
            }
        }
        for (; p < end; ++p) {
            const unsigned e = (unsigned)rev_eid[p];
            const float w = coef[e];
            IpVec<VW> gr;
            gr.load(g + (int64_t)(e / uK) * C + VW * q);
#pragma unroll
            for (int c = 0; c < VW; ++c) acc.v[c] = fmaf(w, gr.v[c], acc.v[c]);
        }
        acc.store(out + j * C + VW * q);
    }
}

}  // namespace crf

using namespace crf;

static bool ip_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" int crfconv_interpolate(const float* src, const float* pos_x, const float* pos_y, const int32_t* idx32, int K,
                                   int64_t n_y, int64_t n_x, int C, float* coef, const int32_t* rev_ptr, const int32_t* rev_eid,
                                   float* out, crf_stream_t stream) {
    CRF_REQUIRE(n_y > 0 && n_y < (int64_t)1 << 31 && n_x > 0 && n_x < (int64_t)1 << 31, CRF_ERR_ARG, "rows n_y=%lld n_x=%lld out of range",
                (long long)n_y, (long long)n_x);
    CRF_REQUIRE(K >= 1 && K <= 64 && C >= 1, CRF_ERR_ARG, "K=%d C=%d invalid (1 <= K <= 64, C >= 1)", K, C);
    CRF_REQUIRE(n_y * K < (int64_t)1 << 31, CRF_ERR_ARG, "edge ids exceed int32 (n_y=%lld K=%d)", (long long)n_y, K);
    CRF_REQUIRE(src && out && out != src, CRF_ERR_ARG, "null pointer or aliasing");
    const bool transpose = rev_ptr != nullptr;
    if (transpose) CRF_REQUIRE(coef && rev_eid && out != coef, CRF_ERR_ARG, "transpose: null pointer or aliasing");
    else CRF_REQUIRE(pos_x && pos_y && idx32 && coef != out && coef != src, CRF_ERR_ARG, "forward: null pointer or aliasing");
    const bool vec = C % 4 == 0 && ip_aligned16(src) && ip_aligned16(out);
    const int CW = vec ? C / 4 : C;                                        // pieces per row
    // forward: four pieces per lane when that is exactly one pass over the row; the transpose keeps one (header)
    const bool four = !transpose && vec && CW % 4 == 0 && CW / 4 <= IP_BLOCK;
    const int per = four ? CW / 4 : CW, lanes = per < IP_BLOCK ? per : IP_BLOCK, rows = IP_BLOCK / lanes;
    const int64_t m = transpose ? n_x : n_y, nblk = cdiv(m, rows);
    CRF_REQUIRE(nblk < (int64_t)1 << 31, CRF_ERR_ARG, "too many workgroups (rows=%lld C=%d)", (long long)m, C);
    const dim3 grid((unsigned)nblk), blk(IP_BLOCK);
    hipStream_t st = as_stream(stream);
    auto forward = [&](auto V, auto P) {
        constexpr int VW = decltype(V)::value, PP = decltype(P)::value;
        dispatch_flag(K == 3 && VW == 4, [&](auto K3) {                 // (the scalar form keeps K a run-time value)
            constexpr int KF = decltype(K3)::value && VW == 4 ? 3 : 0;
            hipLaunchKernelGGL((interp_fwd_kernel<VW, PP, KF>), grid, blk, 0, st, src, pos_x, pos_y, idx32, K, n_y, (int)n_x, C, lanes, coef,
                               out);
        });
    };
    using I1 = std::integral_constant<int, 1>;
    using I4 = std::integral_constant<int, 4>;
    if (transpose)
        dispatch_flag(vec, [&](auto V) {
            hipLaunchKernelGGL(interp_bwd_kernel<decltype(V)::value ? 4 : 1>, grid, blk, 0, st, src, coef, rev_ptr, rev_eid, K, n_x, C, lanes, out);
        });
    else if (four) forward(I4{}, I4{});
    else if (vec) forward(I4{}, I1{});
    else forward(I1{}, I1{});
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
