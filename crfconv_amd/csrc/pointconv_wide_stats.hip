// Forward statistics pass of the wide PointConv layers on the matrix pipe.
// uvstats_kernel's work (pointconv.hip: U = sum_k (h2 - shift) x_j, V = sum_k x_j and the BatchNorm-2 statistic partials of h2 - shift
// from ONE pass over the edges) for K = 16, d in {32, 64, 128} with the d x d layer-2 product of a point's sixteen edges as
// v_mfma_f32_16x16x4_f32 (product (1) of pointconv_wide.hpp; layer 1 evaluated by the lanes in fragment layout).  These launches sit ON
// the chain of the coarse levels (2 560 ... 10 240 points): on the vector ALU a wavefront walked a point's edges four at a time through
// an LDS exchange, 17-21 us per launch whatever the level; here a point is d^2 / 64 MFMAs.
#include "pointconv_wide.hpp"
#include "gridsync.hpp"

namespace crf {

template <int D>
__global__ __launch_bounds__(WP_BLOCK) void uvstats_mfma_kernel(const float* __restrict__ x, const float* __restrict__ pos_src,
                                                                const float* __restrict__ pos_tgt, const int32_t* __restrict__ idx,
                                                                int m, int nblk, const float* __restrict__ A1,
                                                                const float* __restrict__ b1, const float* __restrict__ W2, float slope,
                                                                const float* __restrict__ mean_rel, float* __restrict__ shift_out,
                                                                float* __restrict__ U, float* __restrict__ V, float* __restrict__ partial,
                                                                unsigned* __restrict__ ticket, double* __restrict__ stats) {
    constexpr int T16 = WideTile<D>::T16, S4 = WideTile<D>::S4, LDW = WideTile<D>::LDW;
    constexpr int UNR = S4 > 16 ? 4 : S4;           // k-steps unrolled at a time (fully unrolled, d = 128 runs out of registers)
    __shared__ __attribute__((aligned(16))) float s_w2[D * LDW];
    __shared__ float4 s_a1[D];
    __shared__ float s_shift[D];
    __shared__ float s_h0[D];
    __shared__ float s_red[WP_WAVES][2][D];
    wide_stage_w2<D>(s_w2, W2);
    wide_stage_a1<D>(s_a1, A1, b1);
    for (int c = threadIdx.x; c < D; c += WP_BLOCK) {          // (the rows this thread staged)
        const float4 a = s_a1[c];
        const float pre = fmaf(a.x, mean_rel[0], fmaf(a.y, mean_rel[1], fmaf(a.z, mean_rel[2], a.w)));
        s_h0[c] = pre > 0.f ? pre : slope * pre;
    }
    __syncthreads();
    // shift = layer 2 at the mean relative position (the statistics are taken of h2 - shift: no cancellation in the variance);
    // ascending channel order, the summation order of the vector kernels' h2_of
    for (int c = threadIdx.x; c < D; c += WP_BLOCK) {
        float a = 0.f;
        for (int cp = 0; cp < D; ++cp) a = fmaf(s_h0[cp], s_w2[c * LDW + cp], a);
        s_shift[c] = a;
        if (blockIdx.x == 0) shift_out[c] = a;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = lane & 15, kq = lane >> 4;
    float st1[T16], st2[T16];
#pragma unroll
    for (int tj = 0; tj < T16; ++tj) st1[tj] = st2[tj] = 0.f;
    const int per = (m + nblk - 1) / nblk;
    const int p0 = (int)blockIdx.x * per, p1 = p0 + per < m ? p0 + per : m;
    for (int p = p0 + wave; p < p1; p += WP_WAVES) {
        const WideEdge ed = wide_edge(idx, pos_src, pos_tgt, p, e, kq, true);
        float lv[4];                                 // the rows' flags as factors: a missing edge's results are masked, not its h
#pragma unroll
        for (int r = 0; r < 4; ++r) lv[r] = ed.lr[r] ? 1.f : 0.f;
        float xv[T16][4];
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) {
            wide_x_rows<D>(x, ed, 16 * tj + e, xv[tj]);
#pragma unroll
            for (int r = 0; r < 4; ++r) xv[tj][r] *= lv[r];
        }
        f32x4w acc[T16];                             // acc[tj][r] = h2[edge 4 kq + r][channel 16 tj + e]
        wide_product1<D, T16, UNR, false>(acc, s_w2, s_a1, ed, slope, 0, e, kq, [](int, float) {});
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) {
            const float sh = s_shift[16 * tj + e];
            float u = 0.f, v = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dlt = (acc[tj][r] - sh) * lv[r];
                st1[tj] += dlt;
                st2[tj] = fmaf(dlt, dlt, st2[tj]);
                u = fmaf(dlt, xv[tj][r], u);
                v += xv[tj][r];
            }
            u += __shfl_xor(u, 16, WAVE); u += __shfl_xor(u, 32, WAVE);
            v += __shfl_xor(v, 16, WAVE); v += __shfl_xor(v, 32, WAVE);
            if (kq == 0) {
                U[(int64_t)p * D + 16 * tj + e] = u;
                V[(int64_t)p * D + 16 * tj + e] = v;
            }
        }
    }
#pragma unroll
    for (int tj = 0; tj < T16; ++tj) {
        float a = st1[tj], b = st2[tj];
        a += __shfl_xor(a, 16, WAVE); a += __shfl_xor(a, 32, WAVE);
        b += __shfl_xor(b, 16, WAVE); b += __shfl_xor(b, 32, WAVE);
        if (kq == 0) { s_red[wave][0][16 * tj + e] = a; s_red[wave][1][16 * tj + e] = b; }
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(partial, (int)gridDim.x * 2 * D * 4);
    for (int i = threadIdx.x; i < 2 * D; i += WP_BLOCK) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < WP_WAVES; ++w) a += s_red[w][i / D][i % D];
        st1_sc1(pr, ((int)blockIdx.x * 2 * D + i) * 4, a);       // [block][sum | sum of squares][channel]: block_reduce_store<D, 2>'s layout
    }
    // with a ticket word the last workgroup to finish sums the rows into stats (gridsync.hpp; reduce_partials_kernel's launch otherwise)
    // (its 16 KB of LDS: at d = 128 inside the W2 tile, which every wavefront has left by then -- two workgroups per CU as before)
    constexpr bool ALIAS = sizeof(float) * D * LDW >= sizeof(double) * 4 * WP_BLOCK;
    __shared__ double s_own[ALIAS ? 1 : 4 * WP_BLOCK], s_tot[2 * D];
    __shared__ int s_flag;
    if (ticket == nullptr || !last_workgroup(ticket, gridDim.x, &s_flag)) return;
    double* s_buf = ALIAS ? reinterpret_cast<double*>(s_w2) : s_own;
    sum_partial_rows_f64<WP_BLOCK>(pr, (int)gridDim.x, 2 * D, s_buf, s_tot);
    if (threadIdx.x < 2 * D) stats[threadIdx.x] = s_tot[threadIdx.x];
}

bool uvstats_mfma_ok(int K, int d) {
    return K == 16 && dispatch_width(WIDE_WIDTHS, d, [](auto) {});
}
int uvstats_mfma_launch(const float* x, const float* pos_src, const float* pos_tgt, const int32_t* idx32, int64_t m_tgt, int d,
                        const float* A1, const float* b1, const float* W2, float slope, const float* mean_rel3, float* shift, float* U,
                        float* V, float* partial, int64_t max_blocks, int64_t* nblk_out, unsigned* ticket, double* stats, hipStream_t st) {
    int64_t nb = cdiv(m_tgt, wide_points_per_wave(m_tgt) * WP_WAVES);
    if (nb > max_blocks) nb = max_blocks;
    if (nb < 1) nb = 1;
    *nblk_out = nb;
    const bool known = dispatch_width(WIDE_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(uvstats_mfma_kernel<decltype(D)::value>, dim3((unsigned)nb), dim3(WP_BLOCK), 0, st, x, pos_src, pos_tgt, idx32,
                           (int)m_tgt, (int)nb, A1, b1, W2, slope, mean_rel3, shift, U, V, partial, ticket, stats);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

}  // namespace crf
