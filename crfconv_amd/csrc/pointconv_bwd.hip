// PointConv, the backward passes towards the parameters: BatchNorm-2's reductions over the edges (bwd_reduce_kernel; a training step
// takes them from U and V instead, inside the input-gradient launch of pointconv.hip) and the parameter pass (bwd_params_kernel for
// d <= 16; bwd_dump + a1_reduce around dense GEMMs for wider layers).  Semantics, thread mapping and the shared pieces:
// pointconv_common.hpp.
#include "pointconv_common.hpp"
#include "outer_acc.hpp"

namespace crf {

// ------------------------------------------------------------------ backward pass 1: reductions
template <int D>
__global__ __launch_bounds__(PBLOCK) void bwd_reduce_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ gout,
                                                            const float* __restrict__ pos_src,
                                                            const float* __restrict__ pos_tgt,
                                                            const int32_t* __restrict__ idx, int K,
                                                            int64_t m_tgt, const float* __restrict__ A1,
                                                            const float* __restrict__ b1,
                                                            const float* __restrict__ W2, float slope,
                                                            const float* __restrict__ shift_p,
                                                            float* __restrict__ partial) {
    constexpr int EB = PC<D>::EB;
    __shared__ float4 s_w2t[PC<D>::W2T_F4];
    __shared__ float4 s_scr[PC<D>::SCR_SIZE];
    __shared__ float sred[PWAVES * 2 * D];
    int lane, wave, q;
    const Row rw = my_row<D>(m_tgt, lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    __syncthreads();
    const float4 shift = ld4(shift_p + 4 * q);
    const float px = pos_tgt[3 * rw.r], py = pos_tgt[3 * rw.r + 1], pz = pos_tgt[3 * rw.r + 2];
    const int32_t* irow = idx + rw.r * K;
    float4 g = ld4(gout + rw.r * D + 4 * q);
    if (!rw.valid) g = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    for (int k0 = (wave % PC<D>::KS) * EB; k0 < K; k0 += PC<D>::KS * EB) {
        float4 h1[EB], h2[EB], xj[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const int jj = (k0 + e < K) ? irow[k0 + e] : -1;
            const int64_t j = jj < 0 ? 0 : jj;
            xj[e] = ld4(x + j * D + 4 * q);
            if (jj < 0) xj[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 pre;
            mlp.layer1(px - pos_src[3 * j], py - pos_src[3 * j + 1], pz - pos_src[3 * j + 2], pre, h1[e]);
        }
        mlp.layer2_batch(h1, h2, s_scr);
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const float4 gw = make_float4(g.x * xj[e].x, g.y * xj[e].y, g.z * xj[e].z, g.w * xj[e].w);
            acc[0].x += gw.x; acc[0].y += gw.y; acc[0].z += gw.z; acc[0].w += gw.w;
            acc[1] = make_float4(fmaf(gw.x, h2[e].x - shift.x, acc[1].x), fmaf(gw.y, h2[e].y - shift.y, acc[1].y),
                                 fmaf(gw.z, h2[e].z - shift.z, acc[1].z), fmaf(gw.w, h2[e].w - shift.w, acc[1].w));
        }
    }
    block_reduce_store<D, 2>(acc, sred, partial, lane, wave, q);
}

// ------------------------------------------------------------------ backward pass 2: parameters
// Block partials: float [dW2 D*D] and double [channel][dA1 x, y, z, db1].
template <int D>
__global__ __launch_bounds__(PBLOCK) void bwd_params_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ gout,
                                                            const float* __restrict__ pos_src,
                                                            const float* __restrict__ pos_tgt,
                                                            const int32_t* __restrict__ idx, int K,
                                                            int64_t m_tgt, const float* __restrict__ A1,
                                                            const float* __restrict__ b1,
                                                            const float* __restrict__ W2, float slope,
                                                            const float* __restrict__ ca,
                                                            const float* __restrict__ cb,
                                                            const float* __restrict__ cc,
                                                            float* __restrict__ partial,
                                                            double* __restrict__ partial_d) {
    static_assert(D <= 16, "wider layers go through bwd_dump_kernel / a1_reduce_kernel or pointconv_wide_params.hip");
    constexpr int L = PC<D>::L;
    // dW2 = sum_e g_h2^T h1 -- a reduction over edges of d x d outer products: for d in {8, 16} on the MATRIX pipe (OuterAcc:
    // the wave's g_h2 / h1 rows of one edge per point through a per-wave LDS tile that IS the 16x16x4 fragment layout, four
    // MFMAs per edge round), which takes d FMAs + d/4 broadcasts per lane and edge off the vector ALU and 4 d accumulator
    // registers off the wave (d = 16: 256 -> fewer than 200 registers); d = 4 keeps its four accumulators in registers.
    constexpr bool ACC_MFMA = (D == 8 || D == 16);
    constexpr bool ACC_REGS = !ACC_MFMA;
    constexpr int NSLOT = D * D;
    __shared__ __attribute__((aligned(16))) float s_otile[ACC_MFMA ? 2 * PWAVES * 256 : 4];
    __shared__ float s_ored[ACC_MFMA ? PWAVES * D * D : 1];
    [[maybe_unused]] OuterAcc<ACC_MFMA ? D : 8, PBLOCK> oa;
    __shared__ double s_accd[PWAVES][4 * D];
    __shared__ float4 s_w2t[PC<D>::W2T_F4];
    __shared__ float4 s_w2[D * L];                // W2 rows as float4: s_w2[c * L + q'] = W2[c][4q'..]
    __shared__ float s_acc[NSLOT];                // block totals
    int lane, wave, q;
    const Row rw = my_row<D>(m_tgt, lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    {
        float* s = reinterpret_cast<float*>(s_w2);
        for (int t = threadIdx.x; t < D * D; t += PBLOCK) s[t] = W2[t];
        for (int t = threadIdx.x; t < NSLOT; t += PBLOCK) s_acc[t] = 0.f;
    }
    __syncthreads();
    const float4 va = ld4(ca + 4 * q), vb = ld4(cb + 4 * q), vc = ld4(cc + 4 * q);
    const float px = pos_tgt[3 * rw.r], py = pos_tgt[3 * rw.r + 1], pz = pos_tgt[3 * rw.r + 2];
    const int32_t* irow = idx + rw.r * K;
    float4 g = ld4(gout + rw.r * D + 4 * q);

    float4 dw2[ACC_REGS ? D : 1];  // dw2[c'] = {dW2[4q+0][c'], dW2[4q+1][c'], dW2[4q+2][c'], dW2[4q+3][c']}
    if constexpr (ACC_REGS) {
#pragma unroll
        for (int c = 0; c < D; ++c) dw2[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // dA1 / db1 feed the analytic BatchNorm-1 backward on the host, where their large common
    // components cancel (scale / shift invariance): accumulate them in float64 end to end.
    // Within ONE point (the K edges of this loop) they are summed in float32 -- K terms of like magnitude, relative error
    // ~1e-7 per point, random across points -- and only the sums over points run in float64: the float64 FMAs of the
    // per-edge form were a third of this kernel's vector work.
    float da1[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // [axis][channel of the quad]
    float db[4] = {0, 0, 0, 0};
    const int base = lane - q;

    // PB edges per trip: their index entries first, then all their feature / position rows, then the arithmetic -- two
    // dependent memory phases per PB edges instead of two per edge (one or two wavefronts per SIMD hide nothing)
    constexpr int PB = (D <= 8) ? PARAMS_PB_NARROW : PARAMS_PB;
    for (int k0 = 0; k0 < K; k0 += PB) {
        int jj_[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) jj_[u] = k0 + u < K ? irow[k0 + u] : -1;
        float4 xj_[PB];
        float rx_[PB], ry_[PB], rz_[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const int64_t j = jj_[u] < 0 ? 0 : jj_[u];
            xj_[u] = ld4(x + j * D + 4 * q);
            rx_[u] = px - pos_src[3 * j]; ry_[u] = py - pos_src[3 * j + 1]; rz_[u] = pz - pos_src[3 * j + 2];
        }
#pragma unroll 1
    for (int u = 0; u < PB; ++u) {                  // rolled: the body exists once (unrolled it took 256 + 256 registers);
        const int jj = jj_[0];                      // slot 0 is the current edge, the slots rotate at the end
        const float live = (rw.valid && jj >= 0) ? 1.f : 0.f;
        const float4 xj = xj_[0];
        const float rx = rx_[0], ry = ry_[0], rz = rz_[0];
        float4 pre, h1;
        mlp.layer1(rx, ry, rz, pre, h1);
        const float4 h2 = mlp.layer2(h1);
        // g_h2 for this lane's quad (zero for padding rows and missing neighbours)
        float4 gh2;
        gh2.x = live * fmaf(va.x, g.x * xj.x, fmaf(vb.x, h2.x, vc.x));
        gh2.y = live * fmaf(va.y, g.y * xj.y, fmaf(vb.y, h2.y, vc.y));
        gh2.z = live * fmaf(va.z, g.z * xj.z, fmaf(vb.z, h2.z, vc.z));
        gh2.w = live * fmaf(va.w, g.w * xj.w, fmaf(vb.w, h2.w, vc.w));
        // dW2[quad][c'] += g_h2[quad] * h1[c'] ;  g_h1[quad'] = sum_c g_h2[c] W2[c][quad']
        if constexpr (ACC_MFMA) {
            float* ta = s_otile + wave * 512;
            oa.add_rows(gh2, h1, ta, ta + 256, lane);          // g_h2 is zero for padding rows and missing neighbours
        }
        float4 gh1 = make_float4(0.f, 0.f, 0.f, 0.f);
        static_for<L>([&](auto HQ) {
            constexpr int hq = decltype(HQ)::value;
            const float h0 = group_bcast<L, hq>(h1.x, base), h1b = group_bcast<L, hq>(h1.y, base);
            const float h2b = group_bcast<L, hq>(h1.z, base), h3 = group_bcast<L, hq>(h1.w, base);
            if constexpr (ACC_MFMA) {
                (void)h0; (void)h1b; (void)h2b; (void)h3;                  // (the outer product runs once per edge below)
            } else {
                dw2[4 * hq + 0] = fma4(h0, gh2, dw2[4 * hq + 0]);
                dw2[4 * hq + 1] = fma4(h1b, gh2, dw2[4 * hq + 1]);
                dw2[4 * hq + 2] = fma4(h2b, gh2, dw2[4 * hq + 2]);
                dw2[4 * hq + 3] = fma4(h3, gh2, dw2[4 * hq + 3]);
            }
            const float g0 = group_bcast<L, hq>(gh2.x, base), g1 = group_bcast<L, hq>(gh2.y, base);
            const float g2 = group_bcast<L, hq>(gh2.z, base), g3 = group_bcast<L, hq>(gh2.w, base);
            gh1 = fma4(g0, s_w2[(4 * hq + 0) * L + q], gh1);
            gh1 = fma4(g1, s_w2[(4 * hq + 1) * L + q], gh1);
            gh1 = fma4(g2, s_w2[(4 * hq + 2) * L + q], gh1);
            gh1 = fma4(g3, s_w2[(4 * hq + 3) * L + q], gh1);
        });
        // through lrelu(0.1)
        const float4 gp = make_float4(gh1.x * (pre.x > 0.f ? 1.f : slope), gh1.y * (pre.y > 0.f ? 1.f : slope),
                                      gh1.z * (pre.z > 0.f ? 1.f : slope), gh1.w * (pre.w > 0.f ? 1.f : slope));
        const float gpd[4] = {gp.x, gp.y, gp.z, gp.w};
        const float rd[3] = {rx, ry, rz};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) da1[ax][c] = fmaf(rd[ax], gpd[c], da1[ax][c]);
            db[c] += gpd[c];
        }
#pragma unroll
        for (int v = 0; v + 1 < PB; ++v) {
            jj_[v] = jj_[v + 1]; xj_[v] = xj_[v + 1];
            rx_[v] = rx_[v + 1]; ry_[v] = ry_[v + 1]; rz_[v] = rz_[v + 1];
        }
    }
    }

    // wave-level sums over points, then one LDS add per wave (4 adders per slot, fixed slots)
    if constexpr (ACC_REGS) {
#pragma unroll
        for (int cp = 0; cp < D; ++cp) {
            float4 t = dw2[cp];
            t.x = over_points<D>(t.x); t.y = over_points<D>(t.y);
            t.z = over_points<D>(t.z); t.w = over_points<D>(t.w);
            if (lane < L) {
                atomicAdd(&s_acc[(4 * q + 0) * D + cp], t.x);
                atomicAdd(&s_acc[(4 * q + 1) * D + cp], t.y);
                atomicAdd(&s_acc[(4 * q + 2) * D + cp], t.z);
                atomicAdd(&s_acc[(4 * q + 3) * D + cp], t.w);
            }
        }
    }
    // float64 part: shuffle tree over the wave's points, per-wave LDS slots, fixed-order block sum
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int ax = 0; ax < 4; ++ax) {                       // ax == 3 -> db1
            double t = (double)(ax < 3 ? da1[ax < 3 ? ax : 0][c] : db[c]);
#pragma unroll
            for (int o = L; o < WAVE; o <<= 1) t += __shfl_xor(t, o, WAVE);
            if (lane < L) s_accd[wave][(4 * q + c) * 4 + ax] = t;
        }
    }
    __syncthreads();
    if constexpr (ACC_MFMA) {
        oa.store_partial(s_ored, partial, lane);               // block sum of the waves' accumulators -> partial[block][d * d]
    } else {
        for (int t = threadIdx.x; t < D * D; t += PBLOCK) partial[(int64_t)blockIdx.x * D * D + t] = s_acc[t];
    }
    for (int t = threadIdx.x; t < 4 * D; t += PBLOCK) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < PWAVES; ++w) a += s_accd[w][t];
        partial_d[(int64_t)blockIdx.x * 4 * D + t] = a;        // [channel][x, y, z, bias]
    }
}

// ------------------------------------------------------------------ backward pass 2 for wide layers
// d >= 64 levels have few edges (<= 41k at config 2): write h1, g_h2 and rel per edge and let the
// host contract them with dense GEMMs (dW2 = g_h2^T h1 etc.) instead of reducing d*d sums in-kernel.
template <int D>
__device__ __forceinline__ void bwd_dump_body(const float* __restrict__ x,
                                                          const float* __restrict__ gout,
                                                          const float* __restrict__ pos_src,
                                                          const float* __restrict__ pos_tgt,
                                                          const int32_t* __restrict__ idx, int K,
                                                          int64_t m_tgt, const float* __restrict__ A1,
                                                          const float* __restrict__ b1,
                                                          const float* __restrict__ W2, float slope,
                                                          const float* __restrict__ ca,
                                                          const float* __restrict__ cb,
                                                          const float* __restrict__ cc,
                                                          float* __restrict__ h1_out,
                                                          float* __restrict__ gh2_out,
                                                          float* __restrict__ rel_out, unsigned block) {
    constexpr int EB = PC<D>::EB;
    __shared__ float4 s_w2t[PC<D>::W2T_F4];
    __shared__ float4 s_scr[PC<D>::SCR_SIZE];
    int lane, wave, q;
    const Row rw = my_row_at<D>(m_tgt, block, lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    __syncthreads();
    const float4 va = ld4(ca + 4 * q), vb = ld4(cb + 4 * q), vc = ld4(cc + 4 * q);
    const float px = pos_tgt[3 * rw.r], py = pos_tgt[3 * rw.r + 1], pz = pos_tgt[3 * rw.r + 2];
    const int32_t* irow = idx + rw.r * K;
    const float4 g = ld4(gout + rw.r * D + 4 * q);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = (wave % PC<D>::KS) * EB; k0 < K; k0 += PC<D>::KS * EB) {
        float4 h1[EB], h2[EB], xj[EB];
        float rx[EB], ry[EB], rz[EB];
        bool have[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const int jj = (k0 + e < K) ? irow[k0 + e] : -1;
            have[e] = jj >= 0;
            const int64_t j = have[e] ? jj : 0;
            xj[e] = ld4(x + j * D + 4 * q);
            rx[e] = px - pos_src[3 * j]; ry[e] = py - pos_src[3 * j + 1]; rz[e] = pz - pos_src[3 * j + 2];
            float4 pre;
            mlp.layer1(rx[e], ry[e], rz[e], pre, h1[e]);
        }
        mlp.layer2_batch(h1, h2, s_scr);
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            if (k0 + e >= K || !rw.valid) continue;
            float4 gh2;
            gh2.x = fmaf(va.x, g.x * xj[e].x, fmaf(vb.x, h2[e].x, vc.x));
            gh2.y = fmaf(va.y, g.y * xj[e].y, fmaf(vb.y, h2[e].y, vc.y));
            gh2.z = fmaf(va.z, g.z * xj[e].z, fmaf(vb.z, h2[e].z, vc.z));
            gh2.w = fmaf(va.w, g.w * xj[e].w, fmaf(vb.w, h2[e].w, vc.w));
            const int64_t eid = rw.r * K + k0 + e;
            st4(h1_out + eid * D + 4 * q, have[e] ? h1[e] : zero);
            st4(gh2_out + eid * D + 4 * q, have[e] ? gh2 : zero);
            if (q == 0) {
                rel_out[3 * eid] = have[e] ? rx[e] : 0.f;
                rel_out[3 * eid + 1] = have[e] ? ry[e] : 0.f;
                rel_out[3 * eid + 2] = have[e] ? rz[e] : 0.f;
            }
        }
    }
}

template <int D>
__global__ __launch_bounds__(PBLOCK) void bwd_dump_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                          const float* __restrict__ pos_src, const float* __restrict__ pos_tgt,
                                                          const int32_t* __restrict__ idx, int K, int64_t m_tgt,
                                                          const float* __restrict__ A1, const float* __restrict__ b1,
                                                          const float* __restrict__ W2, float slope, const float* __restrict__ ca,
                                                          const float* __restrict__ cb, const float* __restrict__ cc,
                                                          float* __restrict__ h1_out, float* __restrict__ gh2_out,
                                                          float* __restrict__ rel_out) {
    bwd_dump_body<D>(x, gout, pos_src, pos_tgt, idx, K, m_tgt, A1, b1, W2, slope, ca, cb, cc, h1_out, gh2_out, rel_out, xcd_block_id());
}

// The dump pass of SEVERAL layers of the same width in one launch (the two ResNet blocks of a coarse level: a few workgroups
// each, nothing on the backward chain waits for them -- crfconv_pointconv_wide_params_jobs).
constexpr int PJ_MAX = 8;
struct DumpJobs {
    const float* x[PJ_MAX]; const float* gout[PJ_MAX]; const float* pos_src[PJ_MAX]; const float* pos_tgt[PJ_MAX];
    const int32_t* idx[PJ_MAX];
    const float* A1[PJ_MAX]; const float* b1[PJ_MAX]; const float* W2[PJ_MAX]; const float* ca[PJ_MAX]; const float* cb[PJ_MAX];
    const float* cc[PJ_MAX];
    float* h1[PJ_MAX]; float* gh2[PJ_MAX]; float* rel[PJ_MAX];
    int K[PJ_MAX], m_tgt[PJ_MAX];
    float slope[PJ_MAX];
    int blk_base[PJ_MAX + 1];
    int njobs;
};
template <int D>
__global__ __launch_bounds__(PBLOCK) void bwd_dump_jobs_kernel(const DumpJobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blockIdx.x) ++j;
    bwd_dump_body<D>(t.x[j], t.gout[j], t.pos_src[j], t.pos_tgt[j], t.idx[j], t.K[j], t.m_tgt[j], t.A1[j], t.b1[j], t.W2[j], t.slope[j],
                     t.ca[j], t.cb[j], t.cc[j], t.h1[j], t.gh2[j], t.rel[j], blockIdx.x - (unsigned)t.blk_base[j]);
}

// ------------------------------------------------------------------ backward pass 2b for wide layers
// dA1 | db1 of the dumped path: gp = (g_h2 W2) * lrelu'(h1) per edge, then the four float64 column sums
// sum_e gp[e,c] * {rel_x, rel_y, rel_z, 1}.  gw = g_h2 W2 arrives from a dense GEMM; this is one streaming
// pass over gw / h1 / rel (the float64 elementwise + reduction launches it replaces cost 0.6 ms a step).
template <int D>
__device__ __forceinline__ void a1_reduce_body(const float* __restrict__ gw,
                                                        const float* __restrict__ h1,
                                                        const float* __restrict__ rel, int64_t E, float slope,
                                                        double* __restrict__ partial_d, unsigned block, unsigned nblock) {
    constexpr int L = D / 4, RPB = 256 / L;
    __shared__ double s_acc[256 * 16];
    const int q = threadIdx.x % L, rl = threadIdx.x / L;
    double acc[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[c][t] = 0.0;
    for (int64_t r = (int64_t)block * RPB + rl; r < E; r += (int64_t)nblock * RPB) {
        const float4 a = ld4(gw + r * D + 4 * q), h = ld4(h1 + r * D + 4 * q);
        const double rx = rel[3 * r], ry = rel[3 * r + 1], rz = rel[3 * r + 2];
        const float gp[4] = {a.x * (h.x > 0.f ? 1.f : slope), a.y * (h.y > 0.f ? 1.f : slope),
                             a.z * (h.z > 0.f ? 1.f : slope), a.w * (h.w > 0.f ? 1.f : slope)};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = gp[c];
            acc[c][0] += v * rx; acc[c][1] += v * ry; acc[c][2] += v * rz; acc[c][3] += v;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) s_acc[rl * (4 * D) + (4 * q + c) * 4 + t] = acc[c][t];
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * D; t += 256) {
        double a = 0.0;
        for (int i = 0; i < RPB; ++i) a += s_acc[i * (4 * D) + t];
        partial_d[(int64_t)block * 4 * D + t] = a;        // [channel][x, y, z, bias]
    }
}

template <int D>
__global__ __launch_bounds__(256) void a1_reduce_kernel(const float* __restrict__ gw, const float* __restrict__ h1,
                                                        const float* __restrict__ rel, int64_t E, float slope,
                                                        double* __restrict__ partial_d) {
    a1_reduce_body<D>(gw, h1, rel, E, slope, partial_d, blockIdx.x, gridDim.x);
}
struct A1Jobs {
    const float* gw[PJ_MAX]; const float* h1[PJ_MAX]; const float* rel[PJ_MAX];
    double* partial_d[PJ_MAX];
    int E[PJ_MAX], nblk[PJ_MAX];
    float slope[PJ_MAX];
    int blk_base[PJ_MAX + 1];
    int njobs;
};
template <int D>
__global__ __launch_bounds__(256) void a1_reduce_jobs_kernel(const A1Jobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blockIdx.x) ++j;
    a1_reduce_body<D>(t.gw[j], t.h1[j], t.rel[j], t.E[j], t.slope[j], t.partial_d[j], blockIdx.x - (unsigned)t.blk_base[j], (unsigned)t.nblk[j]);
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_pointconv_bwd_reduce(const float* x, const float* gout, const float* pos_src,
                                            const float* pos_tgt, const int32_t* idx32, int K,
                                            int64_t m_tgt, int d, const float* A1, const float* b1,
                                            const float* W2, float slope, const float* shift, double* red1,
                                            void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(x && gout && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && shift && red1 && workspace,
                CRF_ERR_ARG, "null pointer");
    const int64_t nblk = blocks_for(m_tgt, d);
    CRF_REQUIRE(workspace_bytes >= sizeof(float) * 2 * d * (size_t)nblk, CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>(workspace);
    const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(bwd_reduce_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(PBLOCK), 0, st, x, gout, pos_src,
                           pos_tgt, idx32, K, m_tgt, A1, b1, W2, slope, shift, partial);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return reduce_partials(partial, nblk, 2 * d, red1, st);
}

extern "C" int crfconv_pointconv_bwd_params(const float* x, const float* gout, const float* pos_src,
                                            const float* pos_tgt, const int32_t* idx32, int K,
                                            int64_t m_tgt, int d, const float* A1, const float* b1,
                                            const float* W2, float slope, const float* ca, const float* cb,
                                            const float* cc, double* dW2, double* dA1b1, void* workspace,
                                            size_t workspace_bytes, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(x && gout && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && ca && cb && cc && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE((dW2 == nullptr) == (dA1b1 == nullptr), CRF_ERR_ARG, "dW2 and dA1b1: both or neither (neither = the partial slabs only)");
    CRF_REQUIRE(d <= 16, CRF_ERR_UNSUPPORTED, "in-kernel parameter reduction covers d <= 16; use crfconv_pointconv_bwd_dump for d=%d", d);
    const int64_t nblk = blocks_for(m_tgt, d);
    const size_t fbytes = (sizeof(float) * (size_t)d * d * (size_t)nblk + 255) & ~(size_t)255;
    const size_t dbytes = sizeof(double) * 4 * (size_t)d * (size_t)nblk;
    CRF_REQUIRE(workspace_bytes >= fbytes + dbytes + 256, CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    float* partial = reinterpret_cast<float*>(base);
    double* partial_d = reinterpret_cast<double*>(base + fbytes);
    const bool known = dispatch_width(Widths<4, 8, 16>{}, d, [&](auto D) {
        hipLaunchKernelGGL(bwd_params_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(PBLOCK), 0, st, x, gout, pos_src, pos_tgt,
                           idx32, K, m_tgt, A1, b1, W2, slope, ca, cb, cc, partial, partial_d);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16}", d);
    CRF_LAUNCH_CHECK();
    if (dW2 == nullptr) return CRF_OK;                   // the caller sums the slabs later (crfconv_pointconv_bwd_params_slabs)
    if (int rc = reduce_partials(partial, nblk, d * d, dW2, st)) return rc;
    return reduce_partials_d(partial_d, nblk, 4 * d, dA1b1, st);
}

// Where crfconv_pointconv_bwd_params left its partial slabs inside `workspace`: float [nblk][d*d] (dW2) and double [nblk][4d]
// (dA1 | db1) -- for a caller that passed dW2 = dA1b1 = NULL and finishes the sums with crfconv_reduce_jobs_f64.
extern "C" int crfconv_pointconv_bwd_params_slabs(void* workspace, int64_t m_tgt, int d, const float** slab_w2, const double** slab_a1,
                                                  int64_t* nblk_out) {
    CRF_REQUIRE(workspace && slab_w2 && slab_a1 && nblk_out && m_tgt > 0 && d >= 4 && d <= 16, CRF_ERR_ARG, "bad argument");
    const int64_t nblk = blocks_for(m_tgt, d);
    const size_t fbytes = (sizeof(float) * (size_t)d * d * (size_t)nblk + 255) & ~(size_t)255;
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    *slab_w2 = reinterpret_cast<const float*>(base);
    *slab_a1 = reinterpret_cast<const double*>(base + fbytes);
    *nblk_out = nblk;
    return CRF_OK;
}

extern "C" int crfconv_pointconv_bwd_dump(const float* x, const float* gout, const float* pos_src,
                                          const float* pos_tgt, const int32_t* idx32, int K, int64_t m_tgt,
                                          int d, const float* A1, const float* b1, const float* W2, float slope,
                                          const float* ca, const float* cb, const float* cc, float* h1,
                                          float* gh2, float* rel, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(x && gout && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && ca && cb && cc && h1 && gh2 && rel,
                CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(m_tgt * K < ((int64_t)1 << 31), CRF_ERR_ARG, "too many edges");
    const int64_t nblk = blocks_for(m_tgt, d);
    const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(bwd_dump_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(PBLOCK), 0, as_stream(stream), x, gout,
                           pos_src, pos_tgt, idx32, K, m_tgt, A1, b1, W2, slope, ca, cb, cc, h1, gh2, rel);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// crfconv_pointconv_bwd_dump for several layers: one launch per width present among the jobs (the two ResNet blocks of a level
// share one), workgroups of the jobs laid end to end.  Identical h1 / gh2 / rel.  jobs: host array.
extern "C" int crfconv_pointconv_bwd_dump_jobs(const crf_pc_dump_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j = 0; j < njobs; ++j) {
        const crf_pc_dump_job& jb = jobs[j];
        if (int rc = check_pc(jb.m_tgt, jb.K, jb.d)) return rc;
        CRF_REQUIRE(jb.x && jb.gout && jb.pos_src && jb.pos_tgt && jb.idx32 && jb.A1 && jb.b1 && jb.W2 && jb.ca && jb.cb && jb.cc && jb.h1 &&
                        jb.gh2 && jb.rel, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(jb.m_tgt * jb.K < ((int64_t)1 << 31), CRF_ERR_ARG, "job %d: too many edges", j);
    }
    static const int widths[6] = {4, 8, 16, 32, 64, 128};
    for (int w = 0; w < 6; ++w) {
        const int d = widths[w];
        int j = 0;
        while (j < njobs) {
            DumpJobs t;
            int n = 0;
            int64_t blocks = 0;
            for (; j < njobs && n < PJ_MAX; ++j) {
                const crf_pc_dump_job& jb = jobs[j];
                if (jb.d != d) continue;
                t.x[n] = jb.x; t.gout[n] = jb.gout; t.pos_src[n] = jb.pos_src; t.pos_tgt[n] = jb.pos_tgt; t.idx[n] = jb.idx32;
                t.A1[n] = jb.A1; t.b1[n] = jb.b1; t.W2[n] = jb.W2; t.ca[n] = jb.ca; t.cb[n] = jb.cb; t.cc[n] = jb.cc;
                t.h1[n] = jb.h1; t.gh2[n] = jb.gh2; t.rel[n] = jb.rel; t.K[n] = jb.K; t.m_tgt[n] = (int)jb.m_tgt; t.slope[n] = jb.slope;
                t.blk_base[n] = (int)blocks;
                blocks += blocks_for(jb.m_tgt, d);
                ++n;
            }
            if (n == 0) break;
            for (int k = n; k <= PJ_MAX; ++k) t.blk_base[k] = (int)blocks;
            for (int k = n; k < PJ_MAX; ++k) {
                t.x[k] = t.gout[k] = t.pos_src[k] = t.pos_tgt[k] = t.A1[k] = t.b1[k] = t.W2[k] = t.ca[k] = t.cb[k] = t.cc[k] = nullptr;
                t.idx[k] = nullptr; t.h1[k] = t.gh2[k] = t.rel[k] = nullptr; t.K[k] = 1; t.m_tgt[k] = 0; t.slope[k] = 1.f;
            }
            t.njobs = n;
            const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
                hipLaunchKernelGGL(bwd_dump_jobs_kernel<decltype(D)::value>, dim3((unsigned)blocks), dim3(PBLOCK), 0, st, t);
            });
            CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
            CRF_LAUNCH_CHECK();
        }
    }
    return CRF_OK;
}

// workgroups of a1_reduce_kernel: 256 / (d / 4) edge rows per trip, about eight trips each
static int64_t a1_blocks(int64_t n_edges, int d) { return std::min<int64_t>(1024, cdiv(n_edges, 256 / (d / 4) * 8)); }

// crfconv_pointconv_bwd_a1 (slabs only: the sums are the caller's, crfconv_reduce_jobs_f64) for several layers, one launch per
// width.  Each job's workspace as for the one-layer call; slabs at its 256-byte-aligned start.
extern "C" int crfconv_pointconv_bwd_a1_jobs(const crf_pc_a1_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j = 0; j < njobs; ++j) {
        const crf_pc_a1_job& jb = jobs[j];
        CRF_REQUIRE(jb.gw && jb.h1 && jb.rel && jb.workspace, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(jb.d == 8 || jb.d == 16 || jb.d == 32 || jb.d == 64 || jb.d == 128, CRF_ERR_UNSUPPORTED, "job %d: d=%d", j, jb.d);
        CRF_REQUIRE(jb.n_edges > 0 && jb.n_edges < ((int64_t)1 << 31), CRF_ERR_ARG, "job %d: n_edges out of range", j);
        CRF_REQUIRE(jb.workspace_bytes >= crfconv_pointconv_bwd_a1_workspace(jb.n_edges, jb.d), CRF_ERR_WORKSPACE, "job %d: workspace too small", j);
    }
    static const int widths[5] = {8, 16, 32, 64, 128};
    for (int w = 0; w < 5; ++w) {
        const int d = widths[w];
        int j = 0;
        while (j < njobs) {
            A1Jobs t;
            int n = 0;
            int64_t blocks = 0;
            for (; j < njobs && n < PJ_MAX; ++j) {
                const crf_pc_a1_job& jb = jobs[j];
                if (jb.d != d) continue;
                const int64_t nblk = a1_blocks(jb.n_edges, d);
                t.gw[n] = jb.gw; t.h1[n] = jb.h1; t.rel[n] = jb.rel;
                t.partial_d[n] = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(jb.workspace) + 255) & ~(uintptr_t)255);
                t.E[n] = (int)jb.n_edges; t.nblk[n] = (int)nblk; t.slope[n] = jb.slope;
                t.blk_base[n] = (int)blocks;
                blocks += nblk;
                ++n;
            }
            if (n == 0) break;
            for (int k = n; k <= PJ_MAX; ++k) t.blk_base[k] = (int)blocks;
            for (int k = n; k < PJ_MAX; ++k) { t.gw[k] = t.h1[k] = t.rel[k] = nullptr; t.partial_d[k] = nullptr; t.E[k] = 0; t.nblk[k] = 1; t.slope[k] = 1.f; }
            t.njobs = n;
            const bool known = dispatch_width(Widths<8, 16, 32, 64, 128>{}, d, [&](auto D) {
                hipLaunchKernelGGL(a1_reduce_jobs_kernel<decltype(D)::value>, dim3((unsigned)blocks), dim3(256), 0, st, t);
            });
            CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {8, 16, 32, 64, 128}", d);
            CRF_LAUNCH_CHECK();
        }
    }
    return CRF_OK;
}

extern "C" size_t crfconv_pointconv_bwd_a1_workspace(int64_t n_edges, int d) {
    if (n_edges <= 0 || d < 8) return 0;
    return sizeof(double) * 4 * (size_t)d * (size_t)a1_blocks(n_edges, d) + 256;
}

extern "C" int crfconv_pointconv_bwd_a1(const float* gw, const float* h1, const float* rel, int64_t n_edges, int d,
                                        float slope, double* dA1b1, void* workspace, size_t workspace_bytes,
                                        crf_stream_t stream) {
    CRF_REQUIRE(gw && h1 && rel && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(d == 8 || d == 16 || d == 32 || d == 64 || d == 128, CRF_ERR_UNSUPPORTED, "d=%d not in {8, 16, 32, 64, 128}", d);
    CRF_REQUIRE(n_edges > 0 && n_edges < ((int64_t)1 << 31), CRF_ERR_ARG, "n_edges=%lld out of range", (long long)n_edges);
    CRF_REQUIRE(workspace_bytes >= crfconv_pointconv_bwd_a1_workspace(n_edges, d), CRF_ERR_WORKSPACE, "workspace too small");
    const int64_t nblk = a1_blocks(n_edges, d);
    double* partial_d = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    hipStream_t st = as_stream(stream);
    const bool known = dispatch_width(Widths<8, 16, 32, 64, 128>{}, d, [&](auto D) {
        hipLaunchKernelGGL(a1_reduce_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(256), 0, st, gw, h1, rel, n_edges, slope, partial_d);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {8, 16, 32, 64, 128}", d);
    CRF_LAUNCH_CHECK();
    if (dA1b1 == nullptr) return CRF_OK;                 // slabs only: double [nblk][4d] at the 256-byte-aligned start of `workspace`,
                                                         // nblk = crfconv_pointconv_bwd_a1_nblk; summed later by crfconv_reduce_jobs_f64
    return reduce_partials_d(partial_d, nblk, 4 * d, dA1b1, st);
}

extern "C" int64_t crfconv_pointconv_bwd_a1_nblk(int64_t n_edges, int d) {
    if (n_edges <= 0 || d < 8) return 0;
    return a1_blocks(n_edges, d);
}
