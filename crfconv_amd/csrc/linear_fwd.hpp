// linear_fwd_kernel, the row-streaming product of the per-point Linear layers, with its planning helpers and its ONE host launcher
// (lf_launch), shared by the two units that instantiate it: linear.hip (the forward forms, PRO = false) and mlp_bwd.hip (the dX
// product of the fused MLP backward, PRO = true).
#pragma once
#include "common.hpp"
#include "stream_jobs.h"
#include "uv_fold.hpp"

#include <type_traits>

namespace crf {

// ====================================================================== Y = X W^T (+ b) with BN statistics
// The per-point Linear layers at the fine levels: m = 10^4..10^5 rows, Ci, Co <= 128.  One wavefront owns 16 rows
// and all Co outputs; X rows are read ONCE as float4 (lane l: row l & 15, k = 16 c + 4 (l >> 4) + {0..3}), W sits in
// LDS (rows padded by 4 floats: conflict-free ds_read_b128), and each float4 pair feeds four
// v_mfma_f32_16x16x4_f32 steps (step s takes component s of every lane's float4: the k order inside a 16-chunk is
// permuted identically for both operands, which a sum does not notice).  Output tile D[co][row]: lane holds 4
// consecutive co of one row -> one float4 store.  Optional epilogue: per-block shifted sums / sums of squares of
// every output channel, so BatchNorm needs no separate statistics pass over Y.

#ifndef LF_BLOCK_
#define LF_BLOCK_ 256
#endif
constexpr int LF_BLOCK = LF_BLOCK_, LF_WAVES = LF_BLOCK / WAVE;
using f32x4 = __attribute__((ext_vector_type(4))) float;     // (wgrad_body.hpp declares the same alias)

// PRO: the operand is not read but formed while loading (dX of the fused MLP backward): row r, channel k of
//   gY = alpha[k] * lrelu'(a[k] y + b[k]) * X[r][k] + bet[k] * Y2[r][k] + del[k]     (X = gA, Y2 = the Linear's output y)
// pro = [5][Ci] floats a | b | alpha | bet | del, staged in LDS behind the weight slab (Ci % 4 == 0 required).
// VEC4: Ci % 4 == 0 and Co % 4 == 0 -- every access is a 16-byte one and the element-wise tail code does not exist.  (With
// both forms in one kernel the compiler merges the float4 store into the four predicated dword stores of the tail path:
// 4x the store instructions and 3x the write requests, 983 k instead of 328 k per 21 MB -- TCP_TCC_WRITE_REQ.)
// EPI: 0 plain store; 1 (PRO) Y += addend; 2 (not PRO) dropout mask on Y.  Template forms, so that the common kernels keep their
// register budget (as run-time branches the two epilogues cost <2, false> and <4, true> one wavefront per SIMD each).
// 3 (PRO, VEC4) Y = mask(Y + addend; mask_ref, mask_slope), mask(v; ref, s) = ref > 0 ? v : s v -- lrelu_bwd_kernel's (pool.hip): the
// dX of a block whose input is the output of a ResNet join is handed to that join with the join's LeakyReLU mask already applied.
// 4 (not PRO, VEC4, Ci <= 16; a PROLOGUE despite the parameter's name, which is the one free slot of the kernel's template list): the operand is the
// PointConv combine helper(U, V) of uv_fold.hpp, formed when the fragment is loaded (X = U, uv.V = V) and stored to uv.out by the same lane
// -- each row group is streamed by ONE workgroup per column group, the first column group stores; workgroup (0, 0) publishes a2 / b2 / aux2
// and advances BatchNorm-2's running statistics as uv_combine_kernel's workgroup 0 does.  lin_out of a fine-level ResNet block.
// 5 (not PRO; Co % 4 == 0): the eval-mode MLP block in the product's epilogue -- Y = lrelu(add_rn(fmaf(a, y, b), skip), slope) with
// pro = the BatchNorm's [>= 2][Co] coefficient rows a | b, addend = skip [M, Co] (or null: no residual) and slope (1: no activation):
// bn_apply_kernel's / bn_apply_add_kernel's arithmetic (bn.hip) on the accumulator instead of on a stored y.  No statistic records.
constexpr int EPI_NONE = 0, EPI_ADD = 1, EPI_DROPOUT = 2, EPI_ADD_MASK = 3, EPI_UV = 4, EPI_BN_ACT = 5;
// NCH > 0 (round 4; Ci <= 16 NCH, VEC4): the operand fragments of ALL k chunks of a row group are requested at once and those of
// the wavefront's NEXT row group before the current group's products (NCH <= LF_PF_MAX) -- the rolled loop (NCH = 0) pays one
// dependent memory round trip per chunk, eight per group at 128 inputs, with two to four wavefronts per SIMD to hide them.
#ifndef LF_PF_MAX_
#define LF_PF_MAX_ 4
#endif
template <int TCO, bool PRO = false, bool VEC4 = true, int EPI = EPI_NONE, int NCH = 0>  // 16 * TCO output channels per block slab (blockIdx.y picks the slab)
__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                              const float* __restrict__ bias, int64_t M, int Ci, int Co,
                                                              int transpose_w, float* __restrict__ Y,
                                                              float* __restrict__ stat_partial /*[nblk][Co][4] or null*/,
                                                              const float* __restrict__ Y2 = nullptr,
                                                              const float* __restrict__ pro = nullptr, float slope = 1.f,
                                                              const float* __restrict__ Xb = nullptr, int xsplit = 0,
                                                              float* __restrict__ Yb = nullptr, int ysplit = 0,
                                                              const float* __restrict__ addend = nullptr,
                                                              const long long* __restrict__ drop_counter = nullptr,
                                                              unsigned long long drop_seed = 0ull, unsigned drop_threshold = 0u,
                                                              float drop_scale = 1.f,
                                                              const float* __restrict__ mask_ref = nullptr, float mask_slope = 1.f,
                                                              const UvFold uv = UvFold()) {
    static_assert(EPI != EPI_ADD_MASK || (PRO && VEC4), "the masked epilogue is the aligned dX product's");
    static_assert(EPI != EPI_UV || (!PRO && VEC4 && NCH == 1), "the combine prologue is the narrow aligned forward's");
    static_assert(EPI != EPI_BN_ACT || !PRO, "the BatchNorm epilogue is the forward product's");
    constexpr bool UV = EPI == EPI_UV, TWO = PRO || UV;              // TWO: two raw fragments per chunk
    constexpr bool BNA = EPI == EPI_BN_ACT;
    // mask_ref [M, Co] (EPI_ADD_MASK): the saved output of the join in front of this block (this block's own input x)
    // drop_counter (not PRO, one-pointer output): Y = dropout_mask .* (X W^T) * drop_scale with the counter-based mask of
    // common.hpp (element e = row * Co + column) -- the backward of nn.Dropout applied while the gradient of the Linear
    // BEHIND the dropout is written, instead of in a pass of its own over [M, Co].
    // addend [M, Co] (PRO only, one-pointer output): Y = X W^T + addend -- the gradient the other consumer of the block's input
    // sent back, so that autograd's accumulation pass over three [M, Co] tensors never runs.
    // Xb / xsplit: the operand is the column concatenation [X | Xb] split at column xsplit (the fusion layers' torch.cat,
    // never materialised); Yb / ysplit: the output columns >= ysplit go to Yb [M, Co - ysplit] (dX of such a layer).
    // Both splits are multiples of 4.
    extern __shared__ float sW[];                 // [16*TCO][Cip] (+ [5][Cik] prologue coefficients)
    const int Cip = ((Ci + 15) / 16) * 16 + 4;
    const int Cik = ((Ci + 15) / 16) * 16;
    float* sPro = sW + 16 * TCO * Cip;
    [[maybe_unused]] float* sTile = sPro + (PRO ? 5 * Cik : 0);          // [4 waves][16][16 TCO + 4] output staging (TCO >= 2)
    if constexpr (PRO) {
        for (int t = threadIdx.x; t < 5 * Cik; t += LF_BLOCK) {
            const int which = t / Cik, k = t - which * Cik;
            sPro[t] = k < Ci ? pro[which * Ci + k] : 0.f;
        }
    }
    const int co_base = blockIdx.y * 16 * TCO;
    if (!transpose_w && (Ci % 4) == 0) {          // rows of W are contiguous: 16-byte loads
        const int Cip4 = Cip / 4, Ci4 = Ci / 4;
        for (int t = threadIdx.x; t < 16 * TCO * Cip4; t += LF_BLOCK) {
            const int r = t / Cip4, k4 = t - r * Cip4;
            const int co = co_base + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < Co && k4 < Ci4) v = *reinterpret_cast<const float4*>(W + (int64_t)co * Ci + 4 * k4);
            *reinterpret_cast<float4*>(sW + r * Cip + 4 * k4) = v;
        }
    } else {
        for (int t = threadIdx.x; t < 16 * TCO * Cip; t += LF_BLOCK) {
            const int r = t / Cip, k = t - r * Cip;
            const int co = co_base + r;
            float v = 0.f;
            if (co < Co && k < Ci) v = transpose_w ? W[(int64_t)k * Co + co] : W[(int64_t)co * Ci + k];
            sW[t] = v;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, g = lane >> 4;
    const bool vec = (Ci % 4) == 0;
    float bsel[TCO][4];
#pragma unroll
    for (int t = 0; t < TCO; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co_base + 16 * t + 4 * g + e;
            bsel[t][e] = (bias != nullptr && co < Co) ? bias[co] : 0.f;
        }
    // EPI_BN_ACT: the coefficients of the four channels this lane STORES in pass t (the same in every row group): through the staging
    // tile a lane stores float4 number lane + 64 t of the [16][16 TCO] tile, else its own accumulator columns
    [[maybe_unused]] float4 bna[BNA ? TCO : 1], bnb[BNA ? TCO : 1];
    if constexpr (BNA) {
#pragma unroll
        for (int t = 0; t < TCO; ++t) {
            const int co = TCO >= 2 ? co_base + 4 * ((lane + WAVE * t) % (4 * TCO)) : co_base + 16 * t + 4 * g;
            bna[t] = bnb[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < Co) {
                bna[t] = *reinterpret_cast<const float4*>(pro + co);
                bnb[t] = *reinterpret_cast<const float4*>(pro + Co + co);
            }
        }
    }
    // out = lrelu(add_rn(fmaf(a, y, b), skip), slope) on four channels
    [[maybe_unused]] auto bn_act4 = [&](float4 y, const float4 a, const float4 b, const float* skp) -> float4 {
        float4 o = make_float4(fmaf(a.x, y.x, b.x), fmaf(a.y, y.y, b.y), fmaf(a.z, y.z, b.z), fmaf(a.w, y.w, b.w));
        if (skp != nullptr) {
            const float4 k = *reinterpret_cast<const float4*>(skp);
            o = make_float4(add_rn(o.x, k.x), add_rn(o.y, k.y), add_rn(o.z, k.z), add_rn(o.w, k.w));
        }
        if (slope != 1.f) {
            o.x = o.x > 0.f ? o.x : slope * o.x;
            o.y = o.y > 0.f ? o.y : slope * o.y;
            o.z = o.z > 0.f ? o.z : slope * o.z;
            o.w = o.w > 0.f ? o.w : slope * o.w;
        }
        return o;
    };
    float s1[TCO][4], s2[TCO][4], sh[TCO][4];
#pragma unroll
    for (int t = 0; t < TCO; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[t][e] = 0.f; s2[t][e] = 0.f; sh[t][e] = 0.f; }
    bool have_shift = false;
    const int nchunk = (Ci + 15) / 16;

    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // raw operand fragment(s) of chunk c for row r: X (either layout / the two-pointer form), or (gA, y) with PRO
    auto load_raw = [&](int64_t r, bool rv, int c, float4& xa, float4& xb2) {
        const int k0 = 16 * c + 4 * g;
        xa = zero4;
        xb2 = zero4;
        if (!rv || k0 >= Ci) return;
        if constexpr (PRO) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
            xb2 = *reinterpret_cast<const float4*>(Y2 + r * Ci + k0);
        } else if constexpr (UV) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
            xb2 = *reinterpret_cast<const float4*>(uv.V + r * Ci + k0);
        } else if (Xb != nullptr) {
            if (k0 < xsplit) xa = *reinterpret_cast<const float4*>(X + r * xsplit + k0);
            else xa = *reinterpret_cast<const float4*>(Xb + r * (Ci - xsplit) + (k0 - xsplit));
        } else if (VEC4 || vec) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
        } else if constexpr (!VEC4) {
            const float* xp = X + r * Ci;
            xa.x = xp[k0];
            xa.y = k0 + 1 < Ci ? xp[k0 + 1] : 0.f;
            xa.z = k0 + 2 < Ci ? xp[k0 + 2] : 0.f;
            xa.w = k0 + 3 < Ci ? xp[k0 + 3] : 0.f;
        }
    };
    // the MFMA operand of chunk c: the raw fragment, or gY formed from (gA, y) and the staged coefficients
    auto operand = [&](bool rv, int c, float4 gv, float4 yv) -> float4 {
        if constexpr (PRO) {
            const int k0 = 16 * c + 4 * g;
            float4 xv = zero4;
            if (rv && k0 < Ci) {
                const float4 pa = *reinterpret_cast<const float4*>(sPro + k0), pb = *reinterpret_cast<const float4*>(sPro + Cik + k0);
                const float4 al = *reinterpret_cast<const float4*>(sPro + 2 * Cik + k0), be = *reinterpret_cast<const float4*>(sPro + 3 * Cik + k0);
                const float4 de = *reinterpret_cast<const float4*>(sPro + 4 * Cik + k0);
                xv.x = fmaf(al.x * (fmaf(pa.x, yv.x, pb.x) > 0.f ? 1.f : slope), gv.x, fmaf(be.x, yv.x, de.x));
                xv.y = fmaf(al.y * (fmaf(pa.y, yv.y, pb.y) > 0.f ? 1.f : slope), gv.y, fmaf(be.y, yv.y, de.y));
                xv.z = fmaf(al.z * (fmaf(pa.z, yv.z, pb.z) > 0.f ? 1.f : slope), gv.z, fmaf(be.z, yv.z, de.z));
                xv.w = fmaf(al.w * (fmaf(pa.w, yv.w, pb.w) > 0.f ? 1.f : slope), gv.w, fmaf(be.w, yv.w, de.w));
            }
            return xv;
        } else {
            return gv;
        }
    };
    // EPI_UV: this lane's four channels 4 g .. 4 g + 3 are the same in every row group (one chunk): coefficients in registers
    [[maybe_unused]] float4 uva = zero4, uvt = zero4;
    if constexpr (UV) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < Ci) {
            const UvCoef k = uv_coef(threadIdx.x, Ci, uv.stats, uv.shift, uv.gamma, uv.beta, uv.n_edges, uv.eps);
            uv_publish(threadIdx.x, Ci, k, uv.n_edges, uv.run_mean, uv.run_var, uv.momentum, uv.a2, uv.b2, uv.aux2);
        }
        if (4 * g < Ci) {
            float a[4], tv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const UvCoef k = uv_coef(4 * g + e, Ci, uv.stats, uv.shift, uv.gamma, uv.beta, uv.n_edges, uv.eps);
                a[e] = k.a;
                tv[e] = uv_vcoef(k);
            }
            uva = make_float4(a[0], a[1], a[2], a[3]);
            uvt = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
    }
    // the MFMA operand out = helper(U, V) of row r, stored on the way by the first column group (rows / channels past the end stay zero)
    [[maybe_unused]] auto uv_operand = [&](int64_t r, bool rv, float4 u, float4 v) -> float4 {
        if (!rv || 4 * g >= Ci) return zero4;
        const float4 o = uv_out4(uva, uvt, u, v);
        if (blockIdx.y == 0) *reinterpret_cast<float4*>(uv.out + r * Ci + 4 * g) = o;
        return o;
    };
    // (Issuing the operand loads of four row groups in one burst, or prefetching the next group, measured no faster: the
    // write-heavy shapes run at the ~2.7 TB/s HBM WRITE rate -- 163840 x 8 -> 32 moves 21 MB out in 13 us -- not at a
    // per-wavefront latency limit.)
    constexpr int NCA = NCH > 0 ? NCH : 1;
    constexpr bool PF = NCH > 0 && NCH <= LF_PF_MAX_;                 // next group's fragments in flight too
    const int64_t row_stride = (int64_t)gridDim.x * (LF_BLOCK / WAVE) * 16;
    [[maybe_unused]] float4 fa[NCA], fb[TWO ? NCA : 1], na[PF ? NCA : 1], nb[(PF && TWO) ? NCA : 1];
    [[maybe_unused]] auto load_group = [&](int64_t rw0, float4 (&xa)[NCA], float4 (&xb)[TWO ? NCA : 1]) {
        const int64_t rq = rw0 + rr;
        const bool ok = rw0 < M && rq < M;
#pragma unroll
        for (int c = 0; c < NCA; ++c) {
            float4 t0, t1;
            load_raw(rq, ok, c, t0, t1);
            xa[c] = t0;
            if constexpr (TWO) xb[c] = t1;
        }
    };
    if constexpr (PF) load_group(((int64_t)blockIdx.x * (LF_BLOCK / WAVE) + wave) * 16, fa, fb);
    for (int64_t row0 = ((int64_t)blockIdx.x * (LF_BLOCK / WAVE) + wave) * 16; row0 < M; row0 += row_stride) {
        const int64_t r = row0 + rr;
        const bool rv = r < M;
        f32x4 acc[TCO];
#pragma unroll
        for (int t = 0; t < TCO; ++t) acc[t] = f32x4{bsel[t][0], bsel[t][1], bsel[t][2], bsel[t][3]};
        if constexpr (NCH > 0) {
            if constexpr (PF) {
                if constexpr (TWO) load_group(row0 + row_stride, na, nb);
                else load_group(row0 + row_stride, na, fb);
            } else {
                load_group(row0, fa, fb);
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int k0 = 16 * c + 4 * g;
                float4 xv;
                if constexpr (UV) xv = uv_operand(r, rv, fa[c], fb[c]);
                else xv = operand(rv, c, fa[c], fb[PRO ? c : 0]);
#pragma unroll
                for (int t = 0; t < TCO; ++t) {
                    const float4 wv = *reinterpret_cast<const float4*>(sW + (16 * t + rr) * Cip + k0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv.x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv.y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv.z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv.w, acc[t], 0, 0, 0);
                }
            }
            if constexpr (PF) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    fa[c] = na[c];
                    if constexpr (TWO) fb[c] = nb[c];
                }
            }
        } else {
        for (int c = 0; c < nchunk; ++c) {
            const int k0 = 16 * c + 4 * g;
            float4 ra, rb;
            load_raw(r, rv, c, ra, rb);
            const float4 xv = operand(rv, c, ra, rb);
#pragma unroll
            for (int t = 0; t < TCO; ++t) {
                const float4 wv = *reinterpret_cast<const float4*>(sW + (16 * t + rr) * Cip + k0);
                // D[i = co][j = row]: A = W fragment (i = lane & 15), B = X fragment (j = lane & 15)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv.w, acc[t], 0, 0, 0);
            }
        }
        }
        // lane holds Y[row = row0 + rr][co = co_base + 16 t + 4 g + e], e = 0..3
        if constexpr (TCO >= 2) {
            // Stored straight from the accumulators every store instruction writes 64 bytes into each of 16 rows (measured
            // 1.5-1.7 TB/s on write-heavy shapes); through a per-wave LDS tile [16 rows][16 TCO] every instruction writes
            // whole 128 / 256-byte row segments, consecutive lanes consecutive addresses.
            constexpr int TW = 16 * TCO, TLD = TW + 4, F4R = TW / 4;       // tile width, padded row, float4 per row
            float* tile = sTile + wave * 16 * TLD;
#pragma unroll
            for (int t = 0; t < TCO; ++t)
                *reinterpret_cast<float4*>(tile + rr * TLD + 16 * t + 4 * g) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
            __builtin_amdgcn_wave_barrier();               // LDS operations of one wave complete in order
#pragma unroll
            for (int i = 0; i < (16 * F4R) / WAVE; ++i) {
                const int qd = lane + WAVE * i, trow = qd / F4R, tc4 = qd - trow * F4R;
                const int64_t orow = row0 + trow;
                const int co = co_base + 4 * tc4;
                if (orow < M && co < Co) {
                    float4 o4 = *reinterpret_cast<const float4*>(tile + trow * TLD + 4 * tc4);
                    if constexpr (EPI == EPI_ADD) {
                        {
                            if (VEC4 || (Co % 4) == 0) {
                                const float4 a4 = *reinterpret_cast<const float4*>(addend + orow * Co + co);
                                o4.x += a4.x; o4.y += a4.y; o4.z += a4.z; o4.w += a4.w;
                            } else {
                                o4.x += addend[orow * Co + co];
                                if (co + 1 < Co) o4.y += addend[orow * Co + co + 1];
                                if (co + 2 < Co) o4.z += addend[orow * Co + co + 2];
                                if (co + 3 < Co) o4.w += addend[orow * Co + co + 3];
                            }
                        }
                    }
                    if constexpr (EPI == EPI_ADD_MASK) {
                        const float4 a4 = *reinterpret_cast<const float4*>(addend + orow * Co + co);
                        const float4 r4 = *reinterpret_cast<const float4*>(mask_ref + orow * Co + co);
                        o4.x += a4.x; o4.y += a4.y; o4.z += a4.z; o4.w += a4.w;
                        o4.x = r4.x > 0.f ? o4.x : mask_slope * o4.x;
                        o4.y = r4.y > 0.f ? o4.y : mask_slope * o4.y;
                        o4.z = r4.z > 0.f ? o4.z : mask_slope * o4.z;
                        o4.w = r4.w > 0.f ? o4.w : mask_slope * o4.w;
                    }
                    if constexpr (BNA) o4 = bn_act4(o4, bna[i], bnb[i], addend != nullptr ? addend + orow * Co + co : nullptr);
                    if constexpr (EPI == EPI_DROPOUT) {
                        {
                            const unsigned long long ctr = (unsigned long long)drop_counter[0];
                            const unsigned long long e = (unsigned long long)(orow * Co + co);
                            o4.x = dropout_keep(drop_seed, ctr, e, drop_threshold) ? o4.x * drop_scale : 0.f;
                            o4.y = dropout_keep(drop_seed, ctr, e + 1, drop_threshold) ? o4.y * drop_scale : 0.f;
                            o4.z = dropout_keep(drop_seed, ctr, e + 2, drop_threshold) ? o4.z * drop_scale : 0.f;
                            o4.w = dropout_keep(drop_seed, ctr, e + 3, drop_threshold) ? o4.w * drop_scale : 0.f;
                        }
                    }
                    if (Yb != nullptr) {
                        if (co < ysplit) *reinterpret_cast<float4*>(Y + orow * ysplit + co) = o4;
                        else *reinterpret_cast<float4*>(Yb + orow * (Co - ysplit) + (co - ysplit)) = o4;
                    } else if (VEC4 || (Co % 4) == 0) {
                        *reinterpret_cast<float4*>(Y + orow * Co + co) = o4;
                    } else if constexpr (!VEC4) {
                        const float ov[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < Co) Y[orow * Co + co + e] = ov[e];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();               // the tile is rewritten by the next row group
        } else {
#pragma unroll
        for (int t = 0; t < TCO; ++t) {
            const int co = co_base + 16 * t + 4 * g;
            if constexpr (EPI == EPI_ADD) {
                if (rv) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co) acc[t][e] += addend[r * Co + co + e];
                }
            }
            if constexpr (EPI == EPI_ADD_MASK) {
                if (rv && co < Co) {
                    const float4 a4 = *reinterpret_cast<const float4*>(addend + r * Co + co);
                    const float4 r4 = *reinterpret_cast<const float4*>(mask_ref + r * Co + co);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w}, rf[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[t][e] + av[e];
                        acc[t][e] = rf[e] > 0.f ? v : mask_slope * v;
                    }
                }
            }
            if constexpr (BNA) {
                if (rv && co < Co) {
                    const float4 o4 = bn_act4(make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]), bna[t], bnb[t],
                                              addend != nullptr ? addend + r * Co + co : nullptr);
                    acc[t] = f32x4{o4.x, o4.y, o4.z, o4.w};
                }
            }
            if constexpr (EPI == EPI_DROPOUT) {
                if (rv) {
                    const unsigned long long ctr = (unsigned long long)drop_counter[0];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co)
                            acc[t][e] = dropout_keep(drop_seed, ctr, (unsigned long long)(r * Co + co + e), drop_threshold)
                                            ? acc[t][e] * drop_scale : 0.f;
                }
            }
            if (rv) {
                if (Yb != nullptr) {
                    const float4 o4 = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                    if (co < ysplit) *reinterpret_cast<float4*>(Y + r * ysplit + co) = o4;
                    else if (co < Co) *reinterpret_cast<float4*>(Yb + r * (Co - ysplit) + (co - ysplit)) = o4;
                } else if (VEC4) {
                    if (co < Co) *reinterpret_cast<float4*>(Y + r * Co + co) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                } else if (co + 3 < Co && (Co % 4) == 0) {
                    *reinterpret_cast<float4*>(Y + r * Co + co) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                } else if constexpr (!VEC4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co) Y[r * Co + co + e] = acc[t][e];
                }
            }
        }
        }
        if (!BNA && stat_partial != nullptr) {
            if (!have_shift) {   // shift = this wave's first row (lane with rr == 0 of each co group)
#pragma unroll
                for (int t = 0; t < TCO; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sh[t][e] = __shfl(acc[t][e], 16 * g, WAVE);
                have_shift = true;
            }
            if (rv) {
#pragma unroll
                for (int t = 0; t < TCO; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dlt = acc[t][e] - sh[t][e];
                        s1[t][e] += dlt;
                        s2[t][e] = fmaf(dlt, dlt, s2[t][e]);
                    }
            }
        }
    }
    if (!BNA && stat_partial != nullptr) {
        // one record {shift, n, sum, sumsq} per BLOCK and channel: the 16 row-lanes fold by shuffles, the 4 waves
        // through LDS, re-based on wave 0's shift (sum (v - s0) = a + n d, sum (v - s0)^2 = b + 2 d a + n d^2)
        __syncthreads();                                 // sW is dead: reuse it as [4 waves][4][16*TCO]
        float* sw = sW + wave * 4 * 16 * TCO;
        // rows this wave actually accumulated
        int64_t nrows = 0;
        for (int64_t row0 = ((int64_t)blockIdx.x * (LF_BLOCK / WAVE) + wave) * 16; row0 < M;
             row0 += (int64_t)gridDim.x * (LF_BLOCK / WAVE) * 16)
            nrows += (M - row0) < 16 ? (M - row0) : 16;
#pragma unroll
        for (int t = 0; t < TCO; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = s1[t][e], b = s2[t][e];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    a += __shfl_xor(a, o, WAVE);
                    b += __shfl_xor(b, o, WAVE);
                }
                if (rr == 0) {
                    const int cl = 16 * t + 4 * g + e;
                    sw[cl] = sh[t][e];
                    sw[16 * TCO + cl] = (float)nrows;
                    sw[2 * 16 * TCO + cl] = a;
                    sw[3 * 16 * TCO + cl] = b;
                }
            }
        __syncthreads();
        for (int cl = threadIdx.x; cl < 16 * TCO; cl += LF_BLOCK) {
            const int co = co_base + cl;
            if (co >= Co) continue;
            const float s0 = sW[cl];
            double n = 0.0, S1 = 0.0, S2 = 0.0;
            for (int w = 0; w < LF_BLOCK / WAVE; ++w) {
                const float* q = sW + w * 4 * 16 * TCO;
                const double nb = q[16 * TCO + cl];
                if (nb <= 0.0) continue;
                const double d = (double)q[cl] - (double)s0, a = q[2 * 16 * TCO + cl], b = q[3 * 16 * TCO + cl];
                n += nb;
                S1 += a + nb * d;
                S2 += b + 2.0 * d * a + nb * d * d;
            }
            // record layout [block][channel][4]: one aligned 16-byte tuple per (block, channel)
            *reinterpret_cast<float4*>(stat_partial + ((int64_t)blockIdx.x * Co + co) * 4) =
                make_float4(s0, (float)n, (float)S1, (float)S2);
        }
    }
}

// The same statements as a device function of the workgroup's coordinates (bx, by) in a grid of nbx row workgroups: a job's own coordinates
// and block count in linear_fwd_jobs_kernel, whose launch is the jobs' single launches laid end to end.  linear_fwd_body.inc is a COPY of the
// kernel's statements above with blockIdx.x / blockIdx.y / gridDim.x spelled LF_BX / LF_BY / LF_NBX (tests/test_host_stream_jobs.py holds the
// two texts together).  The kernel does not call this function: through a call the register counts of 27 instantiations moved and two dX
// forms lost a wavefront per SIMD (profiles/r31_stream_groups.md).
template <int TCO, bool PRO, bool VEC4, int EPI, int NCH>
__device__ __forceinline__ void linear_fwd_body(const float* __restrict__ X, const float* __restrict__ W,
                                                const float* __restrict__ bias, int64_t M, int Ci, int Co,
                                                int transpose_w, float* __restrict__ Y,
                                                float* __restrict__ stat_partial /*[nblk][Co][4] or null*/,
                                                const float* __restrict__ Y2, const float* __restrict__ pro, float slope,
                                                const float* __restrict__ Xb, int xsplit, float* __restrict__ Yb, int ysplit,
                                                const float* __restrict__ addend, const long long* __restrict__ drop_counter,
                                                unsigned long long drop_seed, unsigned drop_threshold, float drop_scale,
                                                const float* __restrict__ mask_ref, float mask_slope, const UvFold& uv,
                                                const unsigned bx, const unsigned by, const unsigned nbx) {
#define LF_BX bx
#define LF_BY by
#define LF_NBX nbx
#include "linear_fwd_body.inc"
#undef LF_BX
#undef LF_BY
#undef LF_NBX
}

static int lf_blocks(int64_t M) {
    constexpr int cap = 512;   // swept 128..2048 on the training step: 512 (two blocks per CU, half the statistic records of 1024) is the optimum
    int64_t nb = (M + 16 * LF_WAVES - 1) / (16 * LF_WAVES);           // 16 rows per wave and iteration; two blocks per CU keep
    if (nb > cap) nb = cap;               // enough 16-byte loads in flight; one statistics record per block
    return (int)(nb < 1 ? 1 : nb);
}

// Supported when a 16-channel weight slab fits LDS: 16 x (Ci rounded to 16 + 4) floats (+ prologue rows) <= 64 KB, i.e. Ci <= ~1000.
// Output tiles per workgroup and the dynamic LDS of linear_fwd_kernel for k = Ci inputs, Co outputs: weight slab
// [16 tco][Ci rounded to 16, + 4], the five prologue coefficient rows (dX form), the four output staging tiles (tco >= 2).
// 64 output channels per workgroup at most: the 128-channel form (tco = 8) needs 167 + 98 registers with the statistic
// accumulators, i.e. ONE wavefront per SIMD (measured 68 -> 49 us for 163840 x 32 -> 128; 5.85 -> 5.80 ms per step).  The kernel
// is therefore instantiated for tco = 1, 2 and 4 only (lf_launch).
static size_t lf_lds_bytes_at(int Ci, int tco, bool pro) {
    const size_t cip = (size_t)((Ci + 15) / 16) * 16 + 4, cik = cip - 4;
    size_t floats = 16 * (size_t)tco * cip;
    const size_t stats = (size_t)crf::LF_WAVES * 4 * 16 * (size_t)tco;   // the statistics epilogue reuses the slab as [waves][4][16 tco]
    if (floats < stats) floats = stats;
    if (pro) floats += 5 * cik;
    if (tco >= 2) floats += (size_t)crf::LF_WAVES * 16 * (16 * (size_t)tco + 4);
    return sizeof(float) * floats;
}
// Output tiles per workgroup: by Co, then halved until the slab of k = Ci inputs fits 64 KB (256 inputs: 32 channels per
// workgroup, 512: 16 -- the operand rows are then read once per column slab, from L2).
static int lf_tco(int Ci, int Co, bool pro) {
    constexpr int max_tco = 4;
    const int tiles = (Co + 15) / 16;
    int tco = tiles >= max_tco ? max_tco : (tiles >= 2 ? 2 : 1);
    while (tco > 1 && lf_lds_bytes_at(Ci, tco, pro) > 64 * 1024) tco >>= 1;
    return tco;
}
static size_t lf_lds_bytes(int Ci, int Co, bool pro) { return lf_lds_bytes_at(Ci, lf_tco(Ci, Co, pro), pro); }
// k chunks of the hoisted operand loop (linear_fwd_kernel<.., NCH>): Ci <= 128 in 16-byte pieces; else 0 = the rolled loop
static int lf_hoist_chunks(int Ci, bool vec4) {
    if (!vec4 || Ci > 128) return 0;
    const int n = (Ci + 15) / 16;
    return n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : 8));
}

// ---------------------------------------------------------------------- host side: one argument record, one launcher
struct LinearDropout {
    const long long* counter = nullptr;
    unsigned long long seed = 0ull;
    unsigned threshold = 0u;
    float scale = 1.f;
};

// the eval-mode block's epilogue (EPI_BN_ACT): coef = the BatchNorm's coefficient rows a | b, skip [M, Co] or null, slope (1: none)
struct LinearBnAct {
    const float* coef = nullptr;
    const float* skip = nullptr;
    float slope = 1.f;
};

// linear_fwd_kernel's arguments by name, with the kernel's defaults.  A caller fills what its form uses; lf_launch is the only place
// that lists them positionally.  (A record for the HOST: the kernel keeps its __restrict__ pointer parameters.)
struct LfArgs {                                                  // (grouped as the kernel's parameter list is)
    const float* X = nullptr; const float* W = nullptr;          // X [M, Ci] (PRO: gA; EPI_UV: U); W [Co, Ci], or [Ci, Co] with transpose_w
    const float* bias = nullptr; int64_t M = 0; int Ci = 0, Co = 0;
    int transpose_w = 0; float* Y = nullptr;
    float* stat_partial = nullptr;
    const float* Y2 = nullptr;                                   // PRO: the Linear's output y, the [5][Ci] coefficient rows, the LeakyReLU slope
    const float* pro = nullptr; float slope = 1.f;
    const float* Xb = nullptr; int xsplit = 0;                   // operand [X | Xb] split at column xsplit
    float* Yb = nullptr; int ysplit = 0;                         // output columns >= ysplit
    const float* addend = nullptr;                               // EPI_ADD, EPI_ADD_MASK
    LinearDropout drop;                                          // EPI_DROPOUT
    const float* mask_ref = nullptr; float mask_slope = 1.f;     // EPI_ADD_MASK
    LinearBnAct bn;                                              // EPI_BN_ACT: travels in the kernel's pro / slope / addend parameters
    UvFold uv;                                                   // EPI_UV
};

// The instantiations of linear_fwd_kernel that exist; lf_launch refuses every other combination.  TCO is 1, 2 or 4 (lf_tco).  The
// hoisted operand loop (NCH > 0) is the aligned forms', and the dropout epilogue keeps the rolled one.  dX (PRO): no epilogue or the
// addend, and addend + mask when aligned.  Forward: none, dropout, BatchNorm + activation, and the combine prologue on
// <2 | 4, false, true, EPI_UV, 1> alone.
template <int TCO, bool PRO, bool VEC4, int EPI, int NCH>
constexpr bool lf_form() {
    if (EPI == EPI_UV) return !PRO && VEC4 && TCO >= 2 && NCH == 1;
    if (NCH > 0 && (!VEC4 || EPI == EPI_DROPOUT)) return false;
    if (PRO) return EPI == EPI_NONE || EPI == EPI_ADD || (EPI == EPI_ADD_MASK && VEC4);
    return EPI == EPI_NONE || EPI == EPI_DROPOUT || EPI == EPI_BN_ACT;
}

// f(std::integral_constant<int, V>()) for the V among Vs that equals v (none: no call): a run-time value as a template argument
template <int... Vs, class F>
static void lf_pick(int v, F f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}

// The one launch of linear_fwd_kernel: output tiles per workgroup, alignment, hoisted chunks, grid and LDS are planned here, and the
// instantiation follows from them and the caller's epilogue (the caller has checked its own shapes).
template <bool PRO>
static int lf_launch(const LfArgs& a, int epi, crf_stream_t stream) {
    const int tiles = (a.Co + 15) / 16, tco = lf_tco(a.Ci, a.Co, PRO);
    const bool vec4 = (a.Ci % 4) == 0 && (a.Co % 4) == 0;
    const int nch = epi == EPI_DROPOUT ? 0 : lf_hoist_chunks(a.Ci, vec4);       // 1 / 2 / 4 / 8 chunks: the hoisted loop; 0: the rolled one
    const dim3 grid((unsigned)lf_blocks(a.M), (unsigned)((tiles + tco - 1) / tco)), blk(LF_BLOCK);
    const size_t lds = lf_lds_bytes_at(a.Ci, tco, PRO);
    hipStream_t st = as_stream(stream);
    bool launched = false;
    lf_pick<1, 2, 4>(tco, [&](auto T) { lf_pick<0, 1>(vec4, [&](auto V) {
    lf_pick<EPI_NONE, EPI_ADD, EPI_DROPOUT, EPI_ADD_MASK, EPI_UV, EPI_BN_ACT>(epi, [&](auto E) { lf_pick<0, 1, 2, 4, 8>(nch, [&](auto N) {
        constexpr int TCO = decltype(T)::value, EPI = decltype(E)::value, NCH = decltype(N)::value;
        constexpr bool VEC4 = decltype(V)::value != 0, BNA = EPI == EPI_BN_ACT;
        if constexpr (lf_form<TCO, PRO, VEC4, EPI, NCH>()) {
            hipLaunchKernelGGL((linear_fwd_kernel<TCO, PRO, VEC4, EPI, NCH>), grid, blk, lds, st, a.X, a.W, a.bias, a.M, a.Ci, a.Co,
                               a.transpose_w, a.Y, a.stat_partial, a.Y2, BNA ? a.bn.coef : a.pro, BNA ? a.bn.slope : a.slope, a.Xb,
                               a.xsplit, a.Yb, a.ysplit, BNA ? a.bn.skip : a.addend, a.drop.counter, a.drop.seed, a.drop.threshold,
                               a.drop.scale, a.mask_ref, a.mask_slope, a.uv);
            launched = true;
        }
    }); }); }); });
    CRF_REQUIRE(launched, CRF_ERR_UNSUPPORTED, "linear_fwd_kernel has no form pro=%d epi=%d for %d -> %d", (int)PRO, epi, a.Ci, a.Co);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// ---------------------------------------------------------------------- several INDEPENDENT products per launch
// Up to LFJ_MAX jobs whose single launches (lf_launch) are laid end to end in one grid: workgroup blk_base[j] + bx + nbx by of the launch
// is workgroup (bx, by) of job j's own grid of nbx = lf_blocks(M_j) row workgroups, and runs the instantiation that job's launch would --
// the same rows, summation order and statistic records.  A fine-level launch of these widths is a chain of dependent round trips on
// <= 512 workgroups of 36-76 registers: two of them side by side cost about the longer one.  Forms: the forward's <1, false, true, EPI_NONE,
// 1 | 2 | 4> (Co <= 16, Ci <= 64, one operand, no bias) and the dX product's <1 | 2 | 4, true, true, EPI_NONE | EPI_ADD, 1> (k <= 16).
constexpr int LFJ_MAX = 4;                               // (= GG_MAX of gemm_tile.hpp, BA_MAX of bn_records.hip: the group nodes' size)
struct LfJobs {                                          // (slots at or past njobs are never read)
    const float* X[LFJ_MAX]; const float* W[LFJ_MAX]; float* Y[LFJ_MAX]; float* stat[LFJ_MAX];
    const float* Y2[LFJ_MAX]; const float* pro[LFJ_MAX]; const float* addend[LFJ_MAX];
    long long M[LFJ_MAX];
    int Ci[LFJ_MAX], Co[LFJ_MAX], nbx[LFJ_MAX], form[LFJ_MAX];      // form: NCH (forward); 2 TCO + (addend != null) (dX)
    float slope[LFJ_MAX];
    int blk_base[LFJ_MAX + 1];
    int njobs;
};
// workgroup `blk` of the jobs' grids laid end to end (blockIdx.x in linear_fwd_jobs_kernel; behind the hosted tiles in linear.hip's
// linear_fwd_jobs_hosting_kernel)
template <bool PRO>
__device__ __forceinline__ void linear_fwd_jobs_block(const LfJobs& t, const unsigned blk) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= (int)blk) ++j;
    const unsigned local = blk - (unsigned)t.blk_base[j];
    const unsigned nbx = (unsigned)uni(t.nbx[j]);
    const unsigned bx = (unsigned)uni((int)(local % nbx)), by = (unsigned)uni((int)(local / nbx));
    const float* X = uni(t.X[j]); const float* W = uni(t.W[j]); float* Y = uni(t.Y[j]);
    const int64_t M = uni(t.M[j]);
    const int Ci = uni(t.Ci[j]), Co = uni(t.Co[j]), form = uni(t.form[j]);
    if constexpr (!PRO) {
        float* stat = uni(t.stat[j]);
#define LFJ_FWD(NCH) linear_fwd_body<1, false, true, EPI_NONE, NCH>(X, W, nullptr, M, Ci, Co, 0, Y, stat, nullptr, nullptr, 1.f, nullptr, 0, nullptr, 0, \
                                                                    nullptr, nullptr, 0ull, 0u, 1.f, nullptr, 1.f, UvFold(), bx, by, nbx)
        if (form == 1) LFJ_FWD(1);
        else if (form == 2) LFJ_FWD(2);
        else LFJ_FWD(4);
#undef LFJ_FWD
    } else {
        const float* Y2 = uni(t.Y2[j]); const float* pro = uni(t.pro[j]); const float* addend = uni(t.addend[j]);
        const float slope = uni(t.slope[j]);
#define LFJ_DX(TCO, EPI) linear_fwd_body<TCO, true, true, EPI, 1>(X, W, nullptr, M, Ci, Co, 1, Y, nullptr, Y2, pro, slope, nullptr, 0, nullptr, 0, addend, \
                                                                  nullptr, 0ull, 0u, 1.f, nullptr, 1.f, UvFold(), bx, by, nbx)
        switch (form) {
            case 2: LFJ_DX(1, EPI_NONE); break;
            case 3: LFJ_DX(1, EPI_ADD); break;
            case 4: LFJ_DX(2, EPI_NONE); break;
            case 5: LFJ_DX(2, EPI_ADD); break;
            case 8: LFJ_DX(4, EPI_NONE); break;
            default: LFJ_DX(4, EPI_ADD); break;
        }
#undef LFJ_DX
    }
}
template <bool PRO>
__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_jobs_kernel(const LfJobs t) {
    linear_fwd_jobs_block<PRO>(t, blockIdx.x);
}

// Whether linear_fwd_jobs_kernel<PRO> has the form lf_launch<PRO> would pick for this job (a: the arguments of its single launch)
template <bool PRO>
static bool lf_job_ok(const LfArgs& a, int epi) {
    if (a.M < 1 || a.Ci < 1 || a.Co < 1 || (a.Ci % 4) != 0 || (a.Co % 4) != 0) return false;
    if (a.bias != nullptr || a.Xb != nullptr || a.Yb != nullptr || a.mask_ref != nullptr) return false;
    if (lf_lds_bytes(a.Ci, a.Co, PRO) > 64 * 1024) return false;
    const int tco = lf_tco(a.Ci, a.Co, PRO), nch = lf_hoist_chunks(a.Ci, true);
    if (PRO) return a.transpose_w != 0 && nch == 1 && (epi == EPI_NONE || epi == EPI_ADD);
    return a.transpose_w == 0 && epi == EPI_NONE && tco == 1 && a.Co <= 16 && (nch == 1 || nch == 2 || nch == 4);
}

// The job table of one launch: per job the plan of lf_launch (row workgroups, column slabs, instantiation); dynamic LDS is the largest of
// the jobs' sizes (the body lays its slabs out from its own widths).  epi[j]: EPI_NONE, or EPI_ADD with a[j].addend.
template <bool PRO>
static int lf_jobs_plan(const LfArgs* a, const int* epi, int njobs, LfJobs& t, int64_t& blocks, size_t& lds) {
    CRF_REQUIRE(a && njobs >= 1 && njobs <= LFJ_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d)", LFJ_MAX, njobs);
    t = LfJobs{};
    blocks = 0;
    lds = 0;
    for (int j = 0; j < njobs; ++j) {
        const LfArgs& b = a[j];
        CRF_REQUIRE(lf_job_ok<PRO>(b, epi[j]), CRF_ERR_UNSUPPORTED, "job %d: linear_fwd_jobs_kernel has no form pro=%d epi=%d for %lld x %d -> %d", j,
                    (int)PRO, epi[j], (long long)b.M, b.Ci, b.Co);
        const int tiles = (b.Co + 15) / 16, tco = lf_tco(b.Ci, b.Co, PRO);
        t.X[j] = b.X; t.W[j] = b.W; t.Y[j] = b.Y; t.stat[j] = b.stat_partial; t.Y2[j] = b.Y2; t.pro[j] = b.pro;
        t.addend[j] = epi[j] == EPI_ADD ? b.addend : nullptr;
        t.M[j] = (long long)b.M; t.Ci[j] = b.Ci; t.Co[j] = b.Co; t.nbx[j] = lf_blocks(b.M); t.slope[j] = b.slope;
        t.form[j] = PRO ? 2 * tco + (epi[j] == EPI_ADD ? 1 : 0) : lf_hoist_chunks(b.Ci, true);
        t.blk_base[j] = (int)blocks;
        blocks += (int64_t)t.nbx[j] * ((tiles + tco - 1) / tco);
        const size_t need = lf_lds_bytes_at(b.Ci, tco, PRO);
        if (need > lds) lds = need;
    }
    for (int j = njobs; j <= LFJ_MAX; ++j) t.blk_base[j] = (int)blocks;
    t.njobs = njobs;
    return CRF_OK;
}
template <bool PRO>
static int lf_launch_jobs(const LfArgs* a, const int* epi, int njobs, crf_stream_t stream) {
    LfJobs t;
    int64_t blocks;
    size_t lds;
    if (int rc = lf_jobs_plan<PRO>(a, epi, njobs, t, blocks, lds)) return rc;
    hipLaunchKernelGGL((linear_fwd_jobs_kernel<PRO>), dim3((unsigned)blocks), dim3(LF_BLOCK), lds, as_stream(stream), t);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

}  // namespace crf
