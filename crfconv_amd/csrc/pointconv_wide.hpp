// The WIDE PointConv layers (d = 32, 64, 128: the 10 240-, 2 560- and 640-point levels of PointConvBig) on the matrix pipe: the parameter
// gradients in one pass over the edges and without any per-edge tensor in memory (pointconv_wide_params.hip), and the forward
// statistics pass (pointconv_wide_stats.hip).  This header: the description, the tunables and every step the kernels share.
//
// What the parameter pass computes (models/point_conv_big.py:20-23, 37-58, backward of the weight MLP's second layer and of its first
// layer's folded coefficients), per edge e = (target i, neighbour k) with rel = p_i - p_j:
//     h1  = lrelu(A1 rel + b1)                 [d]       layer 1 (BatchNorm-1 folded into A1, b1)
//     h2  = W2 h1                              [d]       layer 2
//     gh2 = ca (g_i x_j) + cb h2 + cc          [d]       gradient wrt h2 with BatchNorm-2's batch-statistic terms (ca, cb, cc per channel)
//     dW2 += gh2 (x) h1                        [d, d]
//     gp  = (W2^T gh2) lrelu'(h1)              [d]       gradient wrt the layer-1 pre-activation
//     dA1 | db1 += gp (x) [rel, 1]             [d, 4]
// Until round 3 the wide layers wrote h1, gh2 and rel per edge (bwd_dump_kernel: 88 MB at d = 32), a GEMM launch formed gh2 W2,
// a third pass (a1_reduce) the [d, 4] sums and the weight-gradient kernel dW2 -- 136 us of the training step for d = 32 and 64.
//
// Here ONE wavefront (d = 128: a pair) takes ONE target point = 16 edges at a time (K = 16: the edges of a point are exactly the 16
// rows of an MFMA tile) and the three d x d products per edge are v_mfma_f32_16x16x4_f32:
//   (1) H2 = H1 W2^T      A = H1 computed by the lanes DIRECTLY in fragment layout (lane (e, k) holds H1[e][4 s + k]), B = W2 from LDS
//   (2) gh2 from H2, in the MFMA result layout, into the GH2 tile
//   (3) GW = GH2 W2       A = GH2 tile (LDS), B = W2 from LDS
//   (4) gp = GW lrelu'(H1) and the [d, 4] sums, in the result layout
//   (5) dW2 += GH2^T H1   A, B = the GH2 / H1 tiles read row-wise from LDS; the accumulators live across the wave's points
// The forward statistics pass is product (1) and its own finish.  Result layout: lane (g, j) holds rows 4 g .. 4 g + 3, column j.
// LDS row strides: d + 4 floats for W2 and the GH2 tile (conflict-free for the A-fragment reads [row = lane % 16][4 s + lane / 16]
// and for the transposed B-fragment reads of (1)), d + 16 for the H1 tile (conflict-free for the row-wise reads of (5)); the
// remaining row-wise reads of a d + 4 tile are two-way conflicted, far below the matrix pipe's pace (2 LDS reads per 8 CU cycles).
// Per workgroup: one float slab [d, d] (dW2) and one float64 slab [d, 4] (dA1 | db1); the sums over workgroups join the batched
// reductions at the end of the backward pass (crfconv_reduce_jobs, crfconv_reduce_jobs_f64).
#pragma once
#include "common.hpp"

namespace crf {

using f32x4w = __attribute__((ext_vector_type(4))) float;
#ifndef WP_BLOCK_
#define WP_BLOCK_ 512         // 8 wavefronts share one W2 staging (swept on the step, one box: 128 threads 4.337 ms, 256 4.297, 512 4.284)
#endif
constexpr int WP_BLOCK = WP_BLOCK_, WP_WAVES = WP_BLOCK / WAVE, WP_PAIRS = WP_WAVES / 2;

// Points per wavefront.  Every workgroup pays a prologue (W2 into LDS, the shift vector) before its first point, and a wavefront walks
// its points one after the other (each a chain index row -> rows -> MFMAs -> stores that only OTHER wavefronts overlap): few points per
// wavefront pay the prologue too often, many leave the chip without wavefronts.  By level size, swept on the training step on one box
// (big, mid, small): (3, 3, 1) 4.292 ms, (4, 4, 1) 4.300, (4, 2, 1) 4.300, (3, 2, 1) 4.300, (3, 3, 2) 4.307, (4, 4, 4) 4.341; without the
// matrix-pipe kernels 4.388:
#ifndef WP_PPW_BIG_
#define WP_PPW_BIG_ 3         // >= 8192 target points (the 10 240-point level)
#endif
#ifndef WP_PPW_MID_
#define WP_PPW_MID_ 3         // >= 2048 (2 560 points)
#endif
#ifndef WP_PPW_SMALL_
#define WP_PPW_SMALL_ 1       // below (640 points: 160 workgroups)
#endif
inline int64_t wide_points_per_wave(int64_t m_tgt) {
    return m_tgt >= 8192 ? WP_PPW_BIG_ : (m_tgt >= 2048 ? WP_PPW_MID_ : WP_PPW_SMALL_);
}

// the widths of the matrix-pipe kernels (dispatch_width: common.hpp)
constexpr Widths<32, 64, 128> WIDE_WIDTHS{};

// the forward statistics pass (pointconv_wide_stats.hip), called by crfconv_pointconv_forward_uv (pointconv.hip)
// 1 when it takes (K, d); *nblk_out: its workgroup count (<= max_blocks partial slabs of 2 d floats)
bool uvstats_mfma_ok(int K, int d);
int uvstats_mfma_launch(const float* x, const float* pos_src, const float* pos_tgt, const int32_t* idx32, int64_t m_tgt, int d,
                        const float* A1, const float* b1, const float* W2, float slope, const float* mean_rel3, float* shift, float* U,
                        float* V, float* partial, int64_t max_blocks, int64_t* nblk_out, unsigned* ticket, double* stats, hipStream_t st);

// Tiles of width D: T16 column tiles of 16 channels, S4 k-steps of 4 channels, the LDS row strides (see above), K edges per point
template <int D>
struct WideTile {
    static constexpr int T16 = D / 16, S4 = D / 4, LDW = D + 4, LDG = D + 4, LDH = D + 16, K = 16;
};

// W2 [D, D] into LDS at row stride LDW (s_w2 16-byte aligned): sixteen bytes per lane where W2 allows it (a slice of a flat parameter
// vector may start anywhere) -- 64 KB per workgroup at d = 128
template <int D>
__device__ __forceinline__ void wide_stage_w2(float* s_w2, const float* __restrict__ W2) {
    constexpr int LDW = WideTile<D>::LDW;
    if ((reinterpret_cast<uintptr_t>(W2) & 15) == 0) {
        for (int i = threadIdx.x; i < D * D / 4; i += WP_BLOCK)
            *reinterpret_cast<float4*>(s_w2 + (i / (D / 4)) * LDW + 4 * (i % (D / 4))) = reinterpret_cast<const float4*>(W2)[i];
    } else {
        for (int i = threadIdx.x; i < D * D; i += WP_BLOCK) s_w2[(i / D) * LDW + (i % D)] = W2[i];
    }
}
// s_a1[c'] = {A1[c'][0..2], b1[c']}; thread t writes the channels t, t + WP_BLOCK, ...
template <int D>
__device__ __forceinline__ void wide_stage_a1(float4* s_a1, const float* __restrict__ A1, const float* __restrict__ b1) {
    for (int c = threadIdx.x; c < D; c += WP_BLOCK) s_a1[c] = make_float4(A1[3 * c], A1[3 * c + 1], A1[3 * c + 2], b1[c]);
}

// The lane's edge of point p.  Lane (e, kq) evaluates layer 1 for H1[e][4 s + kq], s = 0 .. D/4 - 1 (the A-fragment layout): rel and
// live are those of edge e (a missing edge, or a point that is not `active`, reads neighbour 0 and is not live).  In the result layout
// lane (kq, e) owns rows (edges) 4 kq .. 4 kq + 3 and column (channel) 16 tj + e: jr / lr are the neighbours and flags of those rows.
struct WideEdge {
    float rx, ry, rz;
    bool live;
    int jr[4];
    bool lr[4];
};
__device__ __forceinline__ WideEdge wide_edge(const int32_t* __restrict__ idx, const float* __restrict__ pos_src,
                                              const float* __restrict__ pos_tgt, const int p, const int e, const int kq, const bool active) {
    WideEdge ed;
    const int jraw = idx[(int64_t)p * 16 + e];
    ed.live = active && jraw >= 0;
    const int64_t j = ed.live ? jraw : 0;
    ed.rx = pos_tgt[3 * (int64_t)p] - pos_src[3 * j];
    ed.ry = pos_tgt[3 * (int64_t)p + 1] - pos_src[3 * j + 1];
    ed.rz = pos_tgt[3 * (int64_t)p + 2] - pos_src[3 * j + 2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ed.jr[r] = __shfl((int)j, 4 * kq + r, WAVE);            // lanes 0..15 hold the neighbour of edge `lane`
        ed.lr[r] = __shfl(ed.live ? 1 : 0, 4 * kq + r, WAVE) != 0;
    }
    return ed;
}
// {rel x, y, z, 1} of the lane's edge for the rel tile (a zero row for a missing edge)
__device__ __forceinline__ float4 wide_rel1(const WideEdge& ed) {
    return ed.live ? make_float4(ed.rx, ed.ry, ed.rz, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// the feature rows of the lane's four result rows at channel c
template <int D>
__device__ __forceinline__ void wide_x_rows(const float* __restrict__ x, const WideEdge& ed, const int c, float (&xc)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xc[r] = x[(int64_t)ed.jr[r] * D + c];
}

// Layer 1 of the lane's edge for the channel whose row {A1 | b1} is a
__device__ __forceinline__ float wide_layer1(const float4 a, const WideEdge& ed, const float slope) {
    const float pre = fmaf(a.x, ed.rx, fmaf(a.y, ed.ry, fmaf(a.z, ed.rz, a.w)));
    return pre > 0.f ? pre : slope * pre;
}

// (1) H2 = H1 W2^T for the column tiles [t0, t0 + NT): B[k = c'][j = c] = W2[c][c'].  The A fragment of step s IS layer 1 evaluated for
// this lane's (edge, channel 4 s + kq): computed on the fly (five vector instructions against NT MFMAs) and handed to store(s, h).
// MASK: h of a missing edge is zero (the parameter pass; the statistics pass masks its results instead).  UNR k-steps unrolled at a time.
// acc[tj][r] = H2[edge 4 kq + r][channel 16 (t0 + tj) + e]
template <int D, int NT, int UNR, bool MASK, class Store>
__device__ __forceinline__ void wide_product1(f32x4w (&acc)[NT], const float* s_w2, const float4* s_a1, const WideEdge& ed,
                                              const float slope, const int t0, const int e, const int kq, Store&& store) {
    constexpr int S4 = WideTile<D>::S4, LDW = WideTile<D>::LDW;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[tj] = f32x4w{0.f, 0.f, 0.f, 0.f};
#pragma unroll UNR
    for (int s = 0; s < S4; ++s) {
        const float h1 = wide_layer1(s_a1[4 * s + kq], ed, slope);
        const float h = MASK ? (ed.live ? h1 : 0.f) : h1;
        store(s, h);
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
            acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(h, s_w2[(16 * (t0 + tj) + e) * LDW + 4 * s + kq], acc[tj], 0, 0, 0);
    }
}

// (2) gh2 of the lane's four rows at channel c (h2 = one accumulator of (1), gic = gout[p][c], xc = wide_x_rows) into the GH2 tile
template <int D>
__device__ __forceinline__ void wide_gh2(float* tg, const float* s_coef, const f32x4w h2, const float gic, const float (&xc)[4],
                                         const WideEdge& ed, const int c, const int kq) {
    constexpr int LDG = WideTile<D>::LDG;
    const float va = s_coef[c], vb = s_coef[D + c], vc = s_coef[2 * D + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gh = fmaf(va, gic * xc[r], fmaf(vb, h2[r], vc));
        tg[(4 * kq + r) * LDG + c] = ed.lr[r] ? gh : 0.f;
    }
}

// (5) dW2 += GH2^T H1 for the row tiles [t0, t0 + NT) against every column tile: A[i = c][k = edge] = GH2[edge][c],
// B[k = edge][j = c'] = H1[edge][c'].  accW[ti][tj][r] = dW2[c = 16 (t0 + ti) + 4 kq + r][c' = 16 tj + e]
template <int D, int NT, int UNR>
__device__ __forceinline__ void wide_product5(f32x4w (&accW)[NT][D / 16], const float* tg, const float* th, const int t0, const int e,
                                              const int kq) {
    constexpr int T16 = WideTile<D>::T16, LDG = WideTile<D>::LDG, LDH = WideTile<D>::LDH;
#pragma unroll UNR
    for (int s = 0; s < 4; ++s) {
        float af[NT], bf[T16];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) af[ti] = tg[(4 * s + kq) * LDG + 16 * (t0 + ti) + e];
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) bf[tj] = th[(4 * s + kq) * LDH + 16 * tj + e];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < T16; ++tj)
                accW[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ti], bf[tj], accW[ti][tj], 0, 0, 0);
    }
}

// The dW2 block sum: the SLOTS point slots of a workgroup add their accumulators into s_red (rows of LDR floats) in turn -- a fixed
// order, slot 0 first.  Wavefronts of one slot own disjoint rows.  Every thread of the workgroup calls it; nobody reads what s_red
// aliases any more.  LDR = D + 4 puts the four k-groups of a wavefront (rows 4 kq + r) into different banks; with LDR = D they share one.
template <int D, int NT, int SLOTS, int LDR>
__device__ __forceinline__ void wide_dw2_block_sum(float* s_red, const f32x4w (&accW)[NT][D / 16], const int slot, const int t0,
                                                   const int e, const int kq) {
#pragma unroll                  // (left rolled, a turn's LDS reads wait one by one instead of four at a time: 37 -> 43 us for the d = 64 jobs of the step)
    for (int q = 0; q < SLOTS; ++q) {
        if (slot == q) {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < D / 16; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = (16 * (t0 + ti) + 4 * kq + r) * LDR + 16 * tj + e;
                        s_red[o] = (q == 0 ? 0.f : s_red[o]) + accW[ti][tj][r];
                    }
        }
        __syncthreads();
    }
}
// the workgroup's slabs: dW2 [d, d] from s_red, and dA1 | db1 [channel][x, y, z, bias] as the float64 sum over the slots' [d, 4] sums
template <int D, int LDR>
__device__ __forceinline__ void wide_store_dw2(float* __restrict__ out, const float* s_red) {
    for (int i = threadIdx.x; i < D * D; i += WP_BLOCK) out[i] = s_red[(i / D) * LDR + (i % D)];
}
template <int D, int SLOTS, class T>
__device__ __forceinline__ void wide_store_a1(double* __restrict__ outd, const T* s_sum /*[SLOTS][4 D]*/) {
    for (int i = threadIdx.x; i < 4 * D; i += WP_BLOCK) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < SLOTS; ++w) a += (double)s_sum[w * 4 * D + i];
        outd[i] = a;
    }
}

// LDS of one workgroup of the parameter pass at width D with SLOTS point slots (WP_WAVES wavefronts or WP_PAIRS pairs), in floats:
// W2 | {A1 | b1} | ca | cb | cc | one GH2, H1 and rel tile per slot | F64SUMS: one float64 [D, 4] sum per slot.  159 KB at d = 128
// with four pairs.  Constructed for the caller's slot.
template <int D, int SLOTS, bool F64SUMS>
struct WideParamsLds {
    using T = WideTile<D>;
    static constexpr int A1 = D * T::LDW, COEF = A1 + 4 * D, G = COEF + 3 * D, H = G + SLOTS * T::K * T::LDG,
                         REL = H + SLOTS * T::K * T::LDH, SUM = REL + 4 * SLOTS * T::K, FLOATS = SUM + (F64SUMS ? 2 * SLOTS * 4 * D : 0);
    static_assert(A1 % 4 == 0 && REL % 4 == 0 && SUM % 2 == 0, "float4 and double alignment");
    float* w2;            // W2[c][c'], row c padded to LDW; the block sums reuse it once the points are done
    float4* a1;           // {A1[c'][0..2], b1[c']}
    float* coef;          // ca | cb | cc
    float* g;             // GH2 tile of the slot's point [edge][channel]
    float* h;             // H1 tile [edge][channel]
    float4* rel;          // {rel x, y, z, 1} per edge (zero row for a missing edge)
    double* sum;          // [SLOTS][4 D]: dA1 | db1 of the slots' points (F64SUMS)
    __device__ __forceinline__ WideParamsLds(float* lds, const int slot)
        : w2(lds), a1(reinterpret_cast<float4*>(lds + A1)), coef(lds + COEF), g(lds + G + slot * T::K * T::LDG),
          h(lds + H + slot * T::K * T::LDH), rel(reinterpret_cast<float4*>(lds + REL) + slot * T::K),
          sum(reinterpret_cast<double*>(lds + SUM)) {}
};

}  // namespace crf
