// gemm_tile, the tile routine of the small dense products  C [M, N] = A [M, K] · B (+ bias [N]) (+ addend [M, N]),  with what its
// three families share: gemm.hip (the plain product, its eval epilogue BNACT, several products per launch), gemm_stats.hip (STATS: the
// product that leaves BatchNorm statistic records, with the UV operand) and mlp_small_bwd.hip (PRO: the backward of the coarse MLP block).
//
// Both operands go through LDS, fetched with whole-cache-line loads (8 lanes per 128-byte row segment of a 32-wide K chunk;
// 64-byte row pieces read straight into the fragment layout measured 2 TB/s: 46 us for 2560 x 256 x 512), chunks c + 1 and
// c + 2 in registers while chunk c is on the matrix pipe.  Four wavefronts per workgroup, WR x WC, each WM x WN tiles of
// v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation), D[i = n][j = row]:
//   A operand lane l = (rr = l & 15, g = l >> 4):  B-matrix element [k = kc + 4 g + e][n = 16 tn + rr]
//   B operand lane l:                              A-matrix element [row = 16 tm + rr][k = kc + 4 g + e]
//   lane l ends with C[row = 16 tm + rr][n = 16 tn + 4 g + 0..3]: one 16-byte store.
// The B tile keeps the layout its storage order gives for free ([n][k] for B = W [N, K], [k][n] for B = W [K, N]): no
// transposing scalar traffic.  Summation order over k is fixed by the tile shape alone: results are bitwise reproducible.
#pragma once
#include "common.hpp"
#include "gridsync.hpp"
#include "uv_fold.hpp"

namespace crf {

using gf32x4 = __attribute__((ext_vector_type(4))) float;

#ifndef GM_BK_
#define GM_BK_ 32
#endif
#ifndef GM_PF_
#define GM_PF_ 2
#endif
#ifndef GM_WAIT_SLEEP_
#define GM_WAIT_SLEEP_ 4       // s_sleep argument (64 clocks each) between two polls of an in-launch wait
#endif
constexpr int GM_BLOCK = 256, GM_BK = GM_BK_;      // k columns per chunk (a multiple of 16)
constexpr int GM_PF = GM_PF_;                      // operand chunks in flight per workgroup (register sets; even)
static_assert(GM_PF >= 2 && GM_PF % 2 == 0, "an even number of register sets (the LDS buffers alternate)");

// four consecutive floats of which the first `valid` exist (VEC: widths are multiples of 4, so it is all or nothing and the
// address is 16-byte aligned; else element by element -- odd widths such as the 13-class logits)
template <bool VEC>
__device__ __forceinline__ float4 gm_ld4(const float* __restrict__ p, int valid) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
        if (valid > 0) v = *reinterpret_cast<const float4*>(p);
    } else {
        if (valid > 0) v.x = p[0];
        if (valid > 1) v.y = p[1];
        if (valid > 2) v.z = p[2];
        if (valid > 3) v.w = p[3];
    }
    return v;
}

// PRO form (crfconv_mlp_small_backward): the A operand is not read but FORMED while it is loaded -- gY, the gradient in front of a
// train-mode BatchNorm + LeakyReLU, from (gA, Y) and per-channel coefficients: g1 = gA * lrelu'(a y + b), yh = (y - mean) rstd,
// gY = a (g1 - sum g1 / M - yh sum g1 yh / M).  The two channel means come finished from the tile-sum launch (its last workgroup per
// column slab adds the row-tile partials in float64, round 5: until then EVERY workgroup of the product re-summed all of them --
// 98 KB of partials per workgroup at 256 channels, 2 560 workgroups for a 10 240-row layer); the workgroups of the first column
// slab also store the gY tiles they form (the weight gradient needs them).
constexpr int GM_PRO_MAXK = 512;
struct GemmPro {
    const float* Y;            // [M, K] pre-BatchNorm activations
    const float* coef;         // [4][K]: a | b | mean | rstd
    const float* fin;          // [2][K]: sum g1 / M | sum g1 yh / M (zeros for an eval-mode BatchNorm), left by the tile-sum launch
    float slope;
    float* gY;                 // [M, K] out
    // one-launch form (mlp_small_bwd_jobs_kernel): `fin` is written by tile-sum workgroups of the SAME launch.  sync: the job slot's wait
    // block (gridsync.hpp WL_*: replicas of the finished-slab count -- wait for `need` --, exit tickets of the `nprod` product workgroups,
    // the last of which zeroes the block); fail: the sticky word of gridsync.hpp.  sync == nullptr: `fin` was left by an earlier launch.
    unsigned* sync = nullptr;
    unsigned need = 0, nprod = 0;
    unsigned* fail = nullptr;
    // the product's epilogue also applies the LeakyReLU mask of the ResNet join that produced the block's input (mref [M, N]: that
    // join's saved output): C = mref > 0 ? v : mslope v, v = product + addend -- lrelu_bwd_kernel's arithmetic (pool.hip).  NULL: no mask.
    const float* mref = nullptr;
    float mslope = 1.f;
};
constexpr int GM_PRO_LDS = 6 * GM_PRO_MAXK + 4;     // a | b | mean | rstd | sum g1 / M | sum g1 yh / M | one flag word

template <int WM, int WN, int WR, int WC, bool BNK, bool PRO>
constexpr int gemm_lds_floats() {
    constexpr int BM = 16 * WM * WR, BN = 16 * WN * WC;
    return (PRO ? GM_PRO_LDS : 0) + 2 * BM * (GM_BK + 4) + 2 * (BNK ? BN * (GM_BK + 4) : GM_BK * (BN + 4));
}

// STATS form (crfconv_gemm_stats): the epilogue also leaves BatchNorm statistic records of the tile it holds -- one
// {shift, rows, sum (v - shift), sum (v - shift)^2} tuple per 16-row group and output channel, the layout
// crfconv_bn_coef_from_records combines (Chan, float64) -- so the statistics pass over Y never runs.
// UV form (crfconv_gemm_stats_uv; K <= GM_UV_MAXK): the A operand is the PointConv combine helper(U, V) of uv_fold.hpp, formed when a
// chunk is parked (A = U, uv->V = V; coefficients in uvc [2][GM_UV_MAXK], LDS of the caller's) -- lin_out of the ResNet block at the level
// the tiled product serves; the workgroups of column tile 0 store it to uv->out, workgroup (0, 0) publishes as uv_combine_kernel's does.
// BNACT form (crfconv_gemm_bn_act; N % 4 == 0): the eval-mode MLP block in the epilogue -- C = lrelu(add_rn(fmaf(a, v, b), skip), slope),
// v = the product (+ bias), a | b = rows 0 and 1 of pro.coef [>= 2][N], skip = `addend` (or null), slope = pro.slope (1: no activation):
// bn_apply_kernel's / bn_apply_add_kernel's arithmetic (bn.hip) on the accumulator instead of on a stored product.
constexpr int GM_UV_MAXK = 128;
template <int WM, int WN, int WR, int WC, bool BNK, bool VEC, bool PRO, bool STATS, bool UV = false, bool BNACT = false>
__device__ __forceinline__ void gemm_tile(const float* __restrict__ A, const float* __restrict__ B,
                                          const float* __restrict__ bias, const float* __restrict__ addend,
                                          int M, int N, int K, float* __restrict__ C, const GemmPro& pro,
                                          float* __restrict__ stat_rec, const unsigned bx, const unsigned by,
                                          float* __restrict__ lds /*gemm_lds_floats<...>() floats, 16-byte aligned: the kernel's ONE buffer*/,
                                          const unsigned gridx = 0 /*PRO with pro.sync: row tiles of the job*/,
                                          const UvFold* __restrict__ uv = nullptr, float* __restrict__ uvc = nullptr) {
    static_assert(WR * WC * WAVE == GM_BLOCK, "four wavefronts");
    static_assert(!UV || (VEC && !PRO), "the combine prologue: aligned widths, not the dX product");
    static_assert(!PRO || (VEC && !BNK), "the prologue form is the dX product of aligned widths");
    static_assert(!BNACT || (!PRO && !STATS && !UV), "the BatchNorm epilogue belongs to the plain form");
    constexpr int BM = 16 * WM * WR, BN = 16 * WN * WC;
    constexpr int LDA = GM_BK + 4;                      // [BM][LDA]: 16-byte fragment reads along k, 8 lanes cover the 32 banks
    constexpr int LDN = GM_BK + 4;                      // BNK: [BN][LDN], read like A
    constexpr int LDK = BN + 4;                         // else: [GM_BK][LDK], scalar reads of rows 4 g + e: banks 16 g apart
    constexpr int TA = BM * LDA, TB = BNK ? BN * LDN : GM_BK * LDK;
    constexpr int NA4 = BM * GM_BK / 4, NB4 = BN * GM_BK / 4;       // float4 per tile
    constexpr int PA = (NA4 + GM_BLOCK - 1) / GM_BLOCK, PB = (NB4 + GM_BLOCK - 1) / GM_BLOCK;
    // a kernel that serves several tile classes (the job forms) owns one LDS buffer of the largest: static arrays here would add up
    float* const sPro = lds;                            // PRO: a | b | mean | rstd | sum g1 / M | sum g1 yh / M
    float (*sA)[TA] = reinterpret_cast<float (*)[TA]>(lds + (PRO ? GM_PRO_LDS : 0));
    float (*sB)[TB] = reinterpret_cast<float (*)[TB]>(lds + (PRO ? GM_PRO_LDS : 0) + 2 * TA);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, g = lane >> 4;
    const int wr = wave / WC, wc = wave - wr * WC;
    const int m0 = bx * BM, n0 = by * BN;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    struct Regs { float4 a[PA], b[PB], y[(PRO || UV) ? PA : 1]; int kc; };
    auto fetch = [&](int kc, Regs& r) {
        r.kc = kc;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int q = threadIdx.x + GM_BLOCK * i;
            r.a[i] = zero4;
            if constexpr (PRO || UV) r.y[i] = zero4;
            if (NA4 % GM_BLOCK != 0 && q >= NA4) continue;
            const int row = m0 + q / (GM_BK / 4), k = kc + 4 * (q % (GM_BK / 4));
            if (row < M) r.a[i] = gm_ld4<VEC>(A + (int64_t)row * K + k, K - k);
            if constexpr (PRO) {
                if (row < M) r.y[i] = gm_ld4<VEC>(pro.Y + (int64_t)row * K + k, K - k);
            }
            if constexpr (UV) {
                if (row < M) r.y[i] = gm_ld4<VEC>(uv->V + (int64_t)row * K + k, K - k);
            }
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int q = threadIdx.x + GM_BLOCK * i;
            r.b[i] = zero4;
            if (NB4 % GM_BLOCK != 0 && q >= NB4) continue;
            if constexpr (BNK) {
                const int n = n0 + q / (GM_BK / 4), k = kc + 4 * (q % (GM_BK / 4));
                if (n < N) r.b[i] = gm_ld4<VEC>(B + (int64_t)n * K + k, K - k);
            } else {
                const int k = kc + q / (BN / 4), n = n0 + 4 * (q % (BN / 4));
                if (k < K) r.b[i] = gm_ld4<VEC>(B + (int64_t)k * N + n, N - n);
            }
        }
    };
    auto park = [&](int buf, const Regs& r) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int q = threadIdx.x + GM_BLOCK * i;
            if (NA4 % GM_BLOCK != 0 && q >= NA4) continue;
            float4 av = r.a[i];
            if constexpr (PRO) {
                const int row = m0 + q / (GM_BK / 4), k = r.kc + 4 * (q % (GM_BK / 4));
                if (row < M && k < K) {                  // (rows / channels past the end stay zero)
                    const float4 ca = *reinterpret_cast<const float4*>(sPro + k), cb = *reinterpret_cast<const float4*>(sPro + GM_PRO_MAXK + k);
                    const float4 mu = *reinterpret_cast<const float4*>(sPro + 2 * GM_PRO_MAXK + k), rs = *reinterpret_cast<const float4*>(sPro + 3 * GM_PRO_MAXK + k);
                    const float4 c2 = *reinterpret_cast<const float4*>(sPro + 4 * GM_PRO_MAXK + k), c3 = *reinterpret_cast<const float4*>(sPro + 5 * GM_PRO_MAXK + k);
                    const float4 yv = r.y[i];
                    float4 g1 = av;
                    g1.x *= fmaf(ca.x, yv.x, cb.x) > 0.f ? 1.f : pro.slope;
                    g1.y *= fmaf(ca.y, yv.y, cb.y) > 0.f ? 1.f : pro.slope;
                    g1.z *= fmaf(ca.z, yv.z, cb.z) > 0.f ? 1.f : pro.slope;
                    g1.w *= fmaf(ca.w, yv.w, cb.w) > 0.f ? 1.f : pro.slope;
                    av.x = ca.x * (g1.x - c2.x - (yv.x - mu.x) * rs.x * c3.x);
                    av.y = ca.y * (g1.y - c2.y - (yv.y - mu.y) * rs.y * c3.y);
                    av.z = ca.z * (g1.z - c2.z - (yv.z - mu.z) * rs.z * c3.z);
                    av.w = ca.w * (g1.w - c2.w - (yv.w - mu.w) * rs.w * c3.w);
                    if (by == 0) *reinterpret_cast<float4*>(pro.gY + (int64_t)row * K + k) = av;
                }
            }
            if constexpr (UV) {
                const int row = m0 + q / (GM_BK / 4), k = r.kc + 4 * (q % (GM_BK / 4));
                if (row < M && k < K) {                  // (rows / channels past the end stay zero)
                    av = uv_out4(*reinterpret_cast<const float4*>(uvc + k), *reinterpret_cast<const float4*>(uvc + GM_UV_MAXK + k), av, r.y[i]);
                    if (by == 0) *reinterpret_cast<float4*>(uv->out + (int64_t)row * K + k) = av;
                }
            }
            *reinterpret_cast<float4*>(sA[buf] + (q / (GM_BK / 4)) * LDA + 4 * (q % (GM_BK / 4))) = av;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int q = threadIdx.x + GM_BLOCK * i;
            if (NB4 % GM_BLOCK != 0 && q >= NB4) continue;
            if constexpr (BNK) *reinterpret_cast<float4*>(sB[buf] + (q / (GM_BK / 4)) * LDN + 4 * (q % (GM_BK / 4))) = r.b[i];
            else *reinterpret_cast<float4*>(sB[buf] + (q / (BN / 4)) * LDK + 4 * (q % (BN / 4))) = r.b[i];
        }
    };

    gf32x4 acc[WM][WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = n0 + 16 * (wc * WN + j) + 4 * g;
        float4 bv = zero4;
        if (bias != nullptr) bv = gm_ld4<VEC>(bias + n, N - n);
#pragma unroll
        for (int i = 0; i < WM; ++i) acc[i][j] = gf32x4{bv.x, bv.y, bv.z, bv.w};
    }
    auto compute = [&](int buf) {
        const float* ta = sA[buf] + (16 * wr * WM + rr) * LDA + 4 * g;
        const float* tb = BNK ? sB[buf] + (16 * wc * WN + rr) * LDN + 4 * g : sB[buf] + 4 * g * LDK + 16 * wc * WN + rr;
#pragma unroll
        for (int s = 0; s < GM_BK / 16; ++s) {
            float av[WM][4], wv[WN][4];
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                const float4 a4 = *reinterpret_cast<const float4*>(ta + 16 * i * LDA + 16 * s);
                av[i][0] = a4.x; av[i][1] = a4.y; av[i][2] = a4.z; av[i][3] = a4.w;
            }
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if constexpr (BNK) {
                    const float4 w4 = *reinterpret_cast<const float4*>(tb + 16 * j * LDN + 16 * s);
                    wv[j][0] = w4.x; wv[j][1] = w4.y; wv[j][2] = w4.z; wv[j][3] = w4.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) wv[j][e] = tb[(16 * s + e) * LDK + 16 * j];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j][e], av[i][e], acc[i][j], 0, 0, 0);
        }
    };

    const int nchunk = (K + GM_BK - 1) / GM_BK;
    // GM_PF register sets: chunks c + 1 .. c + GM_PF - 1 sit in registers (or are on their way) while chunk c is on the matrix
    // pipe, chunk c + GM_PF is requested as soon as the set of chunk c has been parked.  A 512-input product is sixteen dependent
    // LDS hand-overs; with two sets (rounds 1-4) each of them also was a memory round trip.
    Regs rs[GM_PF];
#pragma unroll
    for (int d = 0; d < GM_PF; ++d)
        if (d == 0 || d < nchunk) fetch(GM_BK * d, rs[d]);
    if constexpr (PRO) {                                 // behind the first operand loads' issue: channel coefficients into LDS
        for (int k = threadIdx.x; k < K; k += GM_BLOCK) {
            sPro[k] = pro.coef[k];
            sPro[GM_PRO_MAXK + k] = pro.coef[K + k];
            sPro[2 * GM_PRO_MAXK + k] = pro.coef[2 * K + k];
            sPro[3 * GM_PRO_MAXK + k] = pro.coef[3 * K + k];
        }
        if (pro.sync == nullptr) {
            for (int k = threadIdx.x; k < K; k += GM_BLOCK) {
                sPro[4 * GM_PRO_MAXK + k] = pro.fin[k];
                sPro[5 * GM_PRO_MAXK + k] = pro.fin[K + k];
            }
        } else {
            // the two channel means come from tile-sum workgroups of this launch (lower workgroup indices: dispatched before this one, they
            // wait for nobody): thread 0 polls its replica of the job's slab count, bounded like the grid barrier's spin
            int* const s_ok = reinterpret_cast<int*>(sPro + 6 * GM_PRO_MAXK);
            if (threadIdx.x == 0) {
                int ok = 1;
                unsigned spins = 0;
                const unsigned* rep = pro.sync + ((bx + by * 7u) % (unsigned)WL_REPL) * FW_LINE;
                while (__hip_atomic_load(rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pro.need) {
                    __builtin_amdgcn_s_sleep(GM_WAIT_SLEEP_);
                    if (++spins > FW_SPIN_LIMIT) {
                        __hip_atomic_store(pro.fail, 0x300u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = 0;
                        break;
                    }
                }
                *s_ok = ok;
            }
            __syncthreads();
            const bool ok = *s_ok != 0;
            const __amdgpu_buffer_rsrc_t fr = make_rsrc(pro.fin, 2 * K * 4);         // written write-through on another CU: read past L2
            for (int k = threadIdx.x; k < K; k += GM_BLOCK) {
                const float c2 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(fr, 4 * k, 0, 16));
                const float c3 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(fr, 4 * (K + k), 0, 16));
                sPro[4 * GM_PRO_MAXK + k] = ok ? c2 : __builtin_nanf("");            // a spin that gave up poisons this workgroup's tiles
                sPro[5 * GM_PRO_MAXK + k] = c3;
            }
        }
        __syncthreads();
    }
    if constexpr (UV) {                                  // behind the first operand loads' issue: one channel per thread
        if ((int)threadIdx.x < K) {
            const int c = threadIdx.x;
            const UvCoef k = uv_coef(c, K, uv->stats, uv->shift, uv->gamma, uv->beta, uv->n_edges, uv->eps);
            uvc[c] = k.a;
            uvc[GM_UV_MAXK + c] = uv_vcoef(k);
            if (bx == 0 && by == 0) uv_publish(c, K, k, uv->n_edges, uv->run_mean, uv->run_var, uv->momentum, uv->a2, uv->b2, uv->aux2);
        }
        __syncthreads();
    }
    park(0, rs[0]);
    __syncthreads();
    // iteration c = cb + d: chunk c sits in LDS buffer d & 1 (GM_PF is even), its register set d is free again and takes chunk
    // c + GM_PF; the set of chunk c + 1 is parked behind the products of chunk c
    for (int cb = 0; cb < nchunk; cb += GM_PF) {
#pragma unroll
        for (int d = 0; d < GM_PF; ++d) {
            const int c = cb + d;
            if (c >= nchunk) break;
            if (c + GM_PF < nchunk) fetch(GM_BK * (c + GM_PF), rs[d]);
            compute(d & 1);
            if (c + 1 < nchunk) {
                park((d + 1) & 1, rs[(d + 1) % GM_PF]);   // that buffer's readers passed the barrier that ended chunk c - 1
                __syncthreads();
            }
        }
    }
    if constexpr (STATS) {
        static_assert(!STATS || (VEC && WM == 1), "statistic records: one 16-row group per wavefront, aligned widths");
        // lane (rr, g) holds rows rr of the group and channels 4 g .. 4 g + 3 of each of its WN tiles: fold the 16 row lanes
        const int row0 = m0 + 16 * wr * WM;                 // first row of this wavefront's group
        const int nrows = row0 < M ? (M - row0 < 16 ? M - row0 : 16) : 0;
        const bool rvalid = rr < nrows;
        const int rec = (int)bx * WR + wr;          // record = 16-row group
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int n = n0 + 16 * (wc * WN + j) + 4 * g;
            float sv[4], s1[4], s2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sv[e] = __shfl(acc[0][j][e], lane & 0x30, WAVE);            // the group's first row: a sample as shift
                const float d = rvalid ? acc[0][j][e] - sv[e] : 0.f;
                s1[e] = d;
                s2[e] = d * d;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    s1[e] += __shfl_xor(s1[e], o, WAVE);
                    s2[e] += __shfl_xor(s2[e], o, WAVE);
                }
            }
            if (rr == 0 && n < N) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    *reinterpret_cast<float4*>(stat_rec + ((int64_t)rec * N + n + e) * 4) = make_float4(sv[e], (float)nrows, s1[e], s2[e]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int row = m0 + 16 * (wr * WM + i) + rr;
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int n = n0 + 16 * (wc * WN + j) + 4 * g;
            if (n >= N) continue;
            float4 o = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            if constexpr (BNACT) {
                const float4 ca = gm_ld4<VEC>(pro.coef + n, N - n), cb = gm_ld4<VEC>(pro.coef + N + n, N - n);
                o = make_float4(fmaf(ca.x, o.x, cb.x), fmaf(ca.y, o.y, cb.y), fmaf(ca.z, o.z, cb.z), fmaf(ca.w, o.w, cb.w));
                if (addend != nullptr) {
                    const float4 k4 = gm_ld4<VEC>(addend + (int64_t)row * N + n, N - n);
                    o = make_float4(add_rn(o.x, k4.x), add_rn(o.y, k4.y), add_rn(o.z, k4.z), add_rn(o.w, k4.w));
                }
                if (pro.slope != 1.f) {
                    o.x = o.x > 0.f ? o.x : pro.slope * o.x;
                    o.y = o.y > 0.f ? o.y : pro.slope * o.y;
                    o.z = o.z > 0.f ? o.z : pro.slope * o.z;
                    o.w = o.w > 0.f ? o.w : pro.slope * o.w;
                }
            } else if (addend != nullptr) {
                const float4 a4 = gm_ld4<VEC>(addend + (int64_t)row * N + n, N - n);
                o.x += a4.x; o.y += a4.y; o.z += a4.z; o.w += a4.w;
            }
            if constexpr (PRO) {
                if (pro.mref != nullptr) {
                    const float4 r4 = gm_ld4<VEC>(pro.mref + (int64_t)row * N + n, N - n);
                    o.x = r4.x > 0.f ? o.x : pro.mslope * o.x;
                    o.y = r4.y > 0.f ? o.y : pro.mslope * o.y;
                    o.z = r4.z > 0.f ? o.z : pro.mslope * o.z;
                    o.w = r4.w > 0.f ? o.w : pro.mslope * o.w;
                }
            }
            float* cp = C + (int64_t)row * N + n;
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(cp) = o;
            } else {
                cp[0] = o.x;
                if (n + 1 < N) cp[1] = o.y;
                if (n + 2 < N) cp[2] = o.z;
                if (n + 3 < N) cp[3] = o.w;
            }
        }
    }
    if constexpr (PRO) {
        // exit tickets in two levels (a burst on one word is served one by one, ~7 ns each); the job's last product workgroup out zeroes
        // the replicas for the next launch -- every other one has left its wait by then
        if (pro.sync != nullptr && threadIdx.x == 0) {
            const unsigned local = bx + by * gridx, g = local % (unsigned)WL_GROUPS;
            const unsigned n_in_group = pro.nprod / WL_GROUPS + (g < pro.nprod % WL_GROUPS ? 1u : 0u);
            unsigned* gt = pro.sync + (WL_REPL + g) * FW_LINE;
            if (__hip_atomic_fetch_add(gt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == n_in_group) {
                __hip_atomic_store(gt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                unsigned* top = pro.sync + (WL_REPL + WL_GROUPS) * FW_LINE;
                const unsigned groups = pro.nprod < (unsigned)WL_GROUPS ? pro.nprod : (unsigned)WL_GROUPS;
                if (__hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == groups) {
                    __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int r = 0; r < WL_REPL; ++r) __hip_atomic_store(pro.sync + r * FW_LINE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// INDEPENDENT coarse-level MLP blocks in one launch (round 5): the STATS product of each job (crfconv_gemm_stats_jobs) and the PRO
// product of each job's backward (crfconv_mlp_small_backward_jobs).  A coarse launch is a dependent chain of memory round trips on
// a grid that covers a fraction of the chip; two blocks whose inputs are both ready -- unary_nn[i] / pairwise_nn[i] of a CRF layer
// (models/continuous_crf_conv_big.py:56-60), shortcut / lin_in of a strided ResNet block (models/point_conv_big.py:79-88) -- run side
// by side for the price of the longer one.  Same tiles, same summation order as the one-job launches.
constexpr int GG_MAX = 4;
// wide[j]: the job's tiles are 32 rows x 64 columns (a wavefront owns 16 x 32: the A fragment feeds two products, half the
// workgroups pay the load -> LDS -> store chain) -- the flop-heavy layers (GM_WIDE_MIN_N_ columns and GM_WIDE_MIN_TILES_ 32 x 32 tiles).
#ifndef GM_WIDE_MIN_N_
#define GM_WIDE_MIN_N_ 128
#endif
#ifndef GM_WIDE_MIN_TILES_
#define GM_WIDE_MIN_TILES_ 1024
#endif
static inline bool gm_wide(int64_t M, int N) { return N >= GM_WIDE_MIN_N_ && ((M + 31) / 32) * (int64_t)((N + 31) / 32) >= GM_WIDE_MIN_TILES_; }

// The tiles of one job of the 32-row forms (the job launches, crfconv_gemm_stats_uv): tiles_x row tiles, each `wide` or 32 columns.
// before: workgroups the launch already has -- the grid stays below 2^31.
struct GmTilePlan { int tiles_x, wide; int64_t tiles; };
static inline int gm_tile_plan(int64_t M, int N, bool may_be_wide, int64_t before, GmTilePlan& p) {
    p.tiles_x = (int)((M + 31) / 32);
    p.wide = may_be_wide && gm_wide(M, N) ? 1 : 0;
    p.tiles = (int64_t)p.tiles_x * ((N + (p.wide ? 63 : 31)) / (p.wide ? 64 : 32));
    CRF_REQUIRE(before + p.tiles < ((int64_t)1 << 31), CRF_ERR_UNSUPPORTED, "too many tiles in one launch");
    return CRF_OK;
}

// The job kernels of the three units each scan for their job (`while (j + 1 < njobs && base[j + 1] <= blk) ++j`) and name both tile
// widths themselves.  A device function is optimised on its own before it is inlined, and every shared form that was tried -- of
// the scan, of the wide / narrow pair, of the PRO product body -- changed the code of kernels of the training step
// (profiles/r15_gemm_split.md), so the copies stay until such a change is wanted for its own sake.

}  // namespace crf
