// PointConv (depth-wise point convolution with a per-edge weight MLP), gfx950.
//
// Reference semantics: models/point_conv_big.py:37-58.  The reference materialises
// [B, N, K, d] tensors for rel-pos, both MLP layers, the gathered features and their product;
// here nothing per-edge ever reaches HBM: every pass re-derives the weight MLP from the two
// 12-byte positions, and train-mode BatchNorm statistics come from dedicated reduction passes.
//
// Thread mapping: the d channels of a target point sit on L = d/4 adjacent lanes (one float4
// each); a 64-lane wavefront carries 64/L points and loops over their K neighbours.  Layer 1
// (3 -> d) is computed per lane for its own quad; layer 2 (d -> d) broadcasts h1 over the L lanes
// with shuffles against float4 rows of W2^T (registers for d <= 16, LDS above).
//
// This header: the tunables, the per-width geometry PC<D>, the weight MLP EdgeMLP<D>, the row / reduction helpers and the host-side
// width dispatch shared by pointconv.hip (convolution passes: forward and input gradient), pointconv_bwd.hip (passes towards the
// parameters) and pointconv_fold.hip (moments, BatchNorm folds, partial-row sums).
#pragma once
#include "common.hpp"
#include "gridsync.hpp"
#include <algorithm>

namespace crf {

// (the tunables below reach more than one unit: build a variant with `scratch/build_variant.sh <name> all -D...`)
#ifndef PARAMS_PB
#define PARAMS_PB 4
#endif
#ifndef UV_GROUP
#define UV_GROUP 4            // edges per trip of the narrow statistics / convolution pass (uvstats_kernel): 2 (round 2) 28.8, 8 27.5, 6 ~26, 4 24.9 us at d = 8
#endif
#ifndef PARAMS_PB_NARROW
#define PARAMS_PB_NARROW 4      // (d <= 8 with eight edges per trip, 240 registers: 51.5 vs 49.2 us -- not the trips)
#endif
constexpr int PBLOCK = 256;
constexpr int PWAVES = PBLOCK / WAVE;

// Wide layers live on the coarse levels (d = 64: 2560 points, d = 128: 1280 points at config 2): with a point on d/4 lanes a
// launch has a few hundred wavefronts, each one walking ALL K edges of its points through the d x d layer-2 product --
// one wavefront per SIMD running serially for 30-50 us (uvstats / bwd_dump / bwd_input at d = 128).  From d = 64 on, KS
// wavefronts of a workgroup therefore share the SAME points and split their edges (wavefront w of a group takes edge
// batches w, w + KS, ...); what a point accumulates is summed across the wavefronts through LDS (ks_sum) or by the block reductions
// that exist anyway.
#ifndef PC_KS_32
#define PC_KS_32 1
#endif
#ifndef PC_KS_64
#define PC_KS_64 4
#endif
#ifndef PC_KS_128
#define PC_KS_128 2          // swept with PC_KS_64 on the training step: (4, 4) 5.285, (2, 2) 5.249, (2, 4) 5.267, (4, 2) 5.235, (1, 2) 5.271 ms
#endif

template <int D>
struct PC {
    static constexpr int L = D / 4;
    static constexpr int PPW = WAVE / L;
    static constexpr int KS = D >= 128 ? PC_KS_128 : (D >= 64 ? PC_KS_64 : (D >= 32 ? PC_KS_32 : 1));       // wavefronts sharing a point's edges (1, 2 or 4)
    static constexpr int PPB = PPW * PWAVES / KS;
#ifndef PC_W2_REGS_MAX_D
#define PC_W2_REGS_MAX_D 8       // layers up to this width keep W2^T in registers (0: every width reads it from LDS)
#endif
#ifndef PC_NARROW_WAVES
#define PC_NARROW_WAVES 1        // minimum waves per SIMD asked for the narrow statistics kernels
#endif
    static constexpr bool W2_IN_REGS = (D <= PC_W2_REGS_MAX_D);
    // W2^T rows in LDS: [D input channels][L + 1 float4] -- one float4 of padding per row, so that the transposing stage
    // (coalesced global reads of W2 rows, scattered LDS writes) spreads over eight banks instead of one
    static constexpr int W2LD = L + 1;
    // narrow layers (d <= 16) whose W2^T lives in LDS keep layer 1's rows {A1[c][0..2], b1[c]} there too (behind W2^T): 16 registers
    static constexpr bool A1_IN_LDS = !W2_IN_REGS && D <= 16;
    static constexpr int W2T_F4 = W2_IN_REGS ? 1 : D * W2LD + (A1_IN_LDS ? D : 0);      // float4 of the kernels' LDS weight array
    // Wide layers evaluate layer 2 for EB = 4 edges at a time: each W2^T row fetched from LDS then feeds 16 FMAs
    // per lane instead of 4, and h1 is exchanged through a per-wave LDS scratch (broadcast reads) instead of
    // one cross-lane shuffle per input channel -- the d x d product becomes VALU-bound instead of LDS-bound.
    static constexpr int EB = (D >= 32) ? 4 : 1;
    static constexpr int SCR_STRIDE = EB * L + 1;                 // float4 units per point (+1: bank spread)
    static constexpr int SCR_SIZE = EB > 1 ? PWAVES * PPW * SCR_STRIDE : 1;
};

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// Per-thread constants of the weight MLP for this lane's channel quad.
template <int D>
struct EdgeMLP {
    static constexpr int L = PC<D>::L;
    float4 a1[4];  // a1[c] = {A1[c][0], A1[c][1], A1[c][2], b1[c]} for the quad's 4 channels
    float4 w2t_reg[PC<D>::W2_IN_REGS ? D : 1];  // W2T[c'][quad] when held in registers
    const float4* w2t_lds;                      // [D][L + 1] float4 rows otherwise (PC<D>::W2LD)
    int lane, q;
    float slope;                                // LeakyReLU slope of layer 1 (0.1 dense, 0.01 sparse twin)

    __device__ __forceinline__ void init(const float* __restrict__ A1, const float* __restrict__ b1,
                                         const float* __restrict__ W2, float4* lds_w2t, int lane_, int q_, float slope_) {
        lane = lane_;
        q = q_;
        slope = slope_;
        if constexpr (PC<D>::A1_IN_LDS) {
            if ((int)threadIdx.x < D)
                lds_w2t[D * PC<D>::W2LD + threadIdx.x] = make_float4(A1[threadIdx.x * 3 + 0], A1[threadIdx.x * 3 + 1], A1[threadIdx.x * 3 + 2], b1[threadIdx.x]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int ch = 4 * q + c;
                a1[c] = make_float4(A1[ch * 3 + 0], A1[ch * 3 + 1], A1[ch * 3 + 2], b1[ch]);
            }
        }
        if constexpr (PC<D>::W2_IN_REGS) {
#pragma unroll
            for (int cp = 0; cp < D; ++cp)  // W2T[cp][4q+c] = W2[4q+c][cp]
                w2t_reg[cp] = make_float4(W2[(4 * q + 0) * D + cp], W2[(4 * q + 1) * D + cp],
                                          W2[(4 * q + 2) * D + cp], W2[(4 * q + 3) * D + cp]);
            w2t_lds = nullptr;
        } else {
            float* s = reinterpret_cast<float*>(lds_w2t);
            // W2 is read the way it lies in memory (consecutive threads, consecutive addresses) and transposed on the way
            // into LDS: staged the other way round -- LDS order, i.e. a 4 D-byte stride between the lanes' global reads --
            // this prologue was ~15 us of every d = 128 kernel (64 KB through 64-line gathers)
            for (int t = threadIdx.x; t < D * D; t += PBLOCK) {
                const int c = t / D, cp = t % D;               // W2[c][cp] -> row cp (input channel), column c (output)
                s[cp * 4 * PC<D>::W2LD + c] = W2[t];
            }
            w2t_lds = lds_w2t;
        }
    }

    // pre-activation and activation of layer 1 for this lane's quad
    __device__ __forceinline__ void layer1(float rx, float ry, float rz, float4& pre, float4& h1) const {
        float4 r0, r1, r2, r3;
        if constexpr (PC<D>::A1_IN_LDS) {
            int ao = 0;
            asm volatile("" : "+v"(ao));                 // (read per edge, as W2^T: see layer2)
            const float4* ar = w2t_lds + D * PC<D>::W2LD + 4 * q + ao;
            r0 = ar[0]; r1 = ar[1]; r2 = ar[2]; r3 = ar[3];
        } else {
            r0 = a1[0]; r1 = a1[1]; r2 = a1[2]; r3 = a1[3];
        }
        pre.x = fmaf(r0.x, rx, fmaf(r0.y, ry, fmaf(r0.z, rz, r0.w)));
        pre.y = fmaf(r1.x, rx, fmaf(r1.y, ry, fmaf(r1.z, rz, r1.w)));
        pre.z = fmaf(r2.x, rx, fmaf(r2.y, ry, fmaf(r2.z, rz, r2.w)));
        pre.w = fmaf(r3.x, rx, fmaf(r3.y, ry, fmaf(r3.z, rz, r3.w)));
        h1 = make_float4(lrelu(pre.x, slope), lrelu(pre.y, slope), lrelu(pre.z, slope), lrelu(pre.w, slope));
    }

    // h2[quad] = sum_c' h1[c'] * W2[quad][c']
    __device__ __forceinline__ float4 layer2(float4 h1) const {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const int base = lane - q;
        static_for<L>([&](auto HQ) {
            constexpr int hq = decltype(HQ)::value;
            const float v0 = group_bcast<L, hq>(h1.x, base);
            const float v1 = group_bcast<L, hq>(h1.y, base);
            const float v2 = group_bcast<L, hq>(h1.z, base);
            const float v3 = group_bcast<L, hq>(h1.w, base);
            if constexpr (PC<D>::W2_IN_REGS) {
                acc = fma4(v0, w2t_reg[4 * hq + 0], acc);
                acc = fma4(v1, w2t_reg[4 * hq + 1], acc);
                acc = fma4(v2, w2t_reg[4 * hq + 2], acc);
                acc = fma4(v3, w2t_reg[4 * hq + 3], acc);
            } else {
                int wo = 0;
                if constexpr (D <= 16) asm volatile("" : "+v"(wo));    // (narrow layers: keep the reads inside the edge loop -- hoisted they are W2 in registers again)
                const float4* w = w2t_lds + wo;
                acc = fma4(v0, w[(4 * hq + 0) * PC<D>::W2LD + q], acc);
                acc = fma4(v1, w[(4 * hq + 1) * PC<D>::W2LD + q], acc);
                acc = fma4(v2, w[(4 * hq + 2) * PC<D>::W2LD + q], acc);
                acc = fma4(v3, w[(4 * hq + 3) * PC<D>::W2LD + q], acc);
            }
        });
        return acc;
    }

    // h2[e] = W2 h1[e] for EB edges of this lane's point at once (scratch: PC<D>::SCR_SIZE float4 in LDS)
    __device__ __forceinline__ void layer2_batch(const float4 (&h1)[PC<D>::EB], float4 (&h2)[PC<D>::EB],
                                                 float4* scratch) const {
        constexpr int EB = PC<D>::EB;
        if constexpr (EB == 1) {
            h2[0] = layer2(h1[0]);
        } else {
            const int wave = threadIdx.x >> 6, pl = lane / L;
            float4* mine = scratch + (wave * PC<D>::PPW + pl) * PC<D>::SCR_STRIDE;
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                mine[e * L + q] = h1[e];
                h2[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            // same-wave LDS traffic is processed in order: the reads below see the writes above
#pragma unroll 2
            for (int cq = 0; cq < L; ++cq) {
                float4 hv[EB];
#pragma unroll
                for (int e = 0; e < EB; ++e) hv[e] = mine[e * L + cq];
                const float4 w0 = w2t_lds[(4 * cq + 0) * PC<D>::W2LD + q], w1 = w2t_lds[(4 * cq + 1) * PC<D>::W2LD + q];
                const float4 w2 = w2t_lds[(4 * cq + 2) * PC<D>::W2LD + q], w3 = w2t_lds[(4 * cq + 3) * PC<D>::W2LD + q];
#pragma unroll
                for (int e = 0; e < EB; ++e) {
                    h2[e] = fma4(hv[e].x, w0, h2[e]);
                    h2[e] = fma4(hv[e].y, w1, h2[e]);
                    h2[e] = fma4(hv[e].z, w2, h2[e]);
                    h2[e] = fma4(hv[e].w, w3, h2[e]);
                }
            }
        }
    }

    __device__ __forceinline__ float4 h2_of(float rx, float ry, float rz) const {
        float4 pre, h1;
        layer1(rx, ry, rz, pre, h1);
        return layer2(h1);
    }
};

struct Row {
    int64_t r;
    bool valid;
};

template <int D>
__device__ __forceinline__ Row my_row_at(int64_t m, unsigned block, int& lane, int& wave, int& q) {
    lane = threadIdx.x & 63;
    wave = threadIdx.x >> 6;
    q = lane % PC<D>::L;
    const int64_t row = (int64_t)block * PC<D>::PPB + (wave / PC<D>::KS) * PC<D>::PPW + lane / PC<D>::L;
    Row o;
    o.valid = row < m;
    o.r = o.valid ? row : m - 1;
    return o;
}
template <int D>
__device__ __forceinline__ Row my_row(int64_t m, int& lane, int& wave, int& q) {
    return my_row_at<D>(m, xcd_block_id(), lane, wave, q);
}

// Sum `v` over all lanes of the wave that share the same quad index q (xor over the point bits).
template <int D>
__device__ __forceinline__ float over_points(float v) {
#pragma unroll
    for (int o = PC<D>::L; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// Sum of a per-lane float4 over the KS wavefronts that share the same points (fixed order w = 0..KS-1); every wavefront
// returns the total.  s_ks: [PWAVES][WAVE] float4 in LDS.  All threads of the workgroup must call it.
template <int D>
__device__ __forceinline__ float4 ks_sum(float4 v, float4* s_ks, int lane, int wave) {
    if constexpr (PC<D>::KS == 1) {
        return v;
    } else {
        __syncthreads();                                   // s_ks may still be read from an earlier call
        s_ks[wave * WAVE + lane] = v;
        __syncthreads();
        const int w0 = wave - wave % PC<D>::KS;            // first wavefront of this group
        float4 t = s_ks[w0 * WAVE + lane];
#pragma unroll
        for (int w = 1; w < PC<D>::KS; ++w) {
            const float4 o = s_ks[(w0 + w) * WAVE + lane];
            t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        return t;
    }
}

// Block-level deterministic reduction of NV per-quad float4 values into partial[block][NV][D].
template <int D, int NV, bool WT = false>      // WT: rows stored write-through, for a last-workgroup sum in the same launch (gridsync.hpp)
__device__ __forceinline__ void block_reduce_store(const float4 (&v)[NV], float* sred /*[PWAVES][NV][D]*/,
                                                   float* __restrict__ partial, int lane, int wave, int q,
                                                   const unsigned bid = blockIdx.x, const unsigned nblk = gridDim.x) {
#pragma unroll
    for (int n = 0; n < NV; ++n) {
        float4 t = v[n];
        t.x = over_points<D>(t.x);
        t.y = over_points<D>(t.y);
        t.z = over_points<D>(t.z);
        t.w = over_points<D>(t.w);
        if (lane < PC<D>::L) st4(sred + (wave * NV + n) * D + 4 * q, t);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NV * D; t += PBLOCK) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < PWAVES; ++w) a += sred[w * NV * D + t];
        if constexpr (WT) st1_sc1(make_rsrc(partial, (int)nblk * NV * D * 4), ((int)bid * NV * D + t) * 4, a);
        else partial[(int64_t)bid * NV * D + t] = a;
    }
}

// BatchNorm-2 backward coefficients of channel c from the two sums: crfconv_pointconv_fold2_bwd's arithmetic, shared with the ticketed
// reduction inside the input-gradient launch (pointconv.hip: uv_bwd_reduce_body)
__device__ __forceinline__ void fold2_bwd_coef(int c, int d, double sum_gw, double sum_raw, const float* __restrict__ shift,
                                               const double* __restrict__ aux2, const float* __restrict__ gamma, double n_edges,
                                               int use_batch, float* __restrict__ ca, float* __restrict__ cb, float* __restrict__ cc,
                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const double mean = aux2[c], rstd = aux2[d + c], g = gamma[c];
    const double sum_gwh = rstd * (sum_raw - (mean - (double)shift[c]) * sum_gw);    // sum g_w * hhat
    dgamma[c] = (float)sum_gwh;
    dbeta[c] = (float)sum_gw;
    ca[c] = (float)(g * rstd);
    if (use_batch) {
        const double mgw = sum_gw / n_edges, mgh = sum_gwh / n_edges;
        cb[c] = (float)(-g * rstd * rstd * mgh);
        cc[c] = (float)(-g * rstd * mgw + g * rstd * rstd * mean * mgh);
    } else {
        cb[c] = 0.f;
        cc[c] = 0.f;
    }
}

// ------------------------------------------------------------------ host side
static int check_pc(int64_t m, int K, int d) {
    CRF_REQUIRE(m > 0 && m < ((int64_t)1 << 31), CRF_ERR_ARG, "rows=%lld out of range", (long long)m);
    CRF_REQUIRE(K >= 1 && K <= 64, CRF_ERR_ARG, "K=%d out of range", K);
    CRF_REQUIRE(d == 4 || d == 8 || d == 16 || d == 32 || d == 64 || d == 128, CRF_ERR_UNSUPPORTED,
                "d=%d not in {4,8,16,32,64,128}", d);
    return CRF_OK;
}

// the PointConv widths (dispatch_width: common.hpp)
constexpr Widths<4, 8, 16, 32, 64, 128> ALL_WIDTHS{};

// workgroups of an edge kernel over m points (0: d is no PointConv width)
template <int D>
constexpr int64_t nblocks_of(int64_t m) { return (m + PC<D>::PPB - 1) / PC<D>::PPB; }
inline int64_t blocks_for(int64_t m, int d) {
    int64_t n = 0;
    dispatch_width(ALL_WIDTHS, d, [&](auto D) { n = nblocks_of<decltype(D)::value>(m); });
    return n;
}

// out[slot] = sum_b partial[b][slot] in float64, fixed order (pointconv_fold.hip: reduce_partials_kernel / reduce_partials_d_kernel)
int reduce_partials(const float* partial, int64_t nblk, int nslots, double* out, hipStream_t st);
int reduce_partials_d(const double* partial, int64_t nblk, int nslots, double* out, hipStream_t st);

}  // namespace crf
