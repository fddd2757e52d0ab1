// Parameter gradients of the wide PointConv layers on the matrix pipe: the two walks over the target points (one wavefront per point
// for d = 32 / 64, a pair of wavefronts per point for d = 128), the one kernel that serves every width, and its entries.
// What is computed, the numbered products (1) to (5), the layouts and every shared step: pointconv_wide.hpp.
#include "pointconv_wide.hpp"
#include "wgrad_body.hpp"

namespace crf {

constexpr int WP_MAX = 8;

struct WideJobs {
    const float* x[WP_MAX]; const float* gout[WP_MAX]; const float* pos_src[WP_MAX]; const float* pos_tgt[WP_MAX];
    const int32_t* idx[WP_MAX];
    const float* A1[WP_MAX]; const float* b1[WP_MAX]; const float* W2[WP_MAX]; const float* ca[WP_MAX]; const float* cb[WP_MAX];
    const float* cc[WP_MAX];
    float* dw2_partial[WP_MAX]; double* a1_partial[WP_MAX];
    int m_tgt[WP_MAX], nblk[WP_MAX], d[WP_MAX];
    float slope[WP_MAX];
    int blk_base[WP_MAX + 1];
    int njobs;
};

// W2, {A1 | b1} and the BatchNorm-2 coefficients of a job into the workgroup's LDS (the caller's barrier follows)
template <int D, class Lds>
__device__ __forceinline__ void wide_params_stage(const Lds& s, const WideJobs& t, const int job) {
    wide_stage_w2<D>(s.w2, t.W2[job]);
    wide_stage_a1<D>(s.a1, t.A1[job], t.b1[job]);
    for (int c = threadIdx.x; c < D; c += WP_BLOCK) {
        s.coef[c] = t.ca[job][c];
        s.coef[D + c] = t.cb[job][c];
        s.coef[2 * D + c] = t.cc[job][c];
    }
}

// d = 32 / 64: one wavefront per target point, stride WP_WAVES over the workgroup's points, wavefront barriers.  (At d = 128 one
// wavefront would hold (d/16)^2 = 64 dW2 tiles = 256 accumulators beside everything else and spill: the pair walk below.)
template <int D>
using WideLds1 = WideParamsLds<D, WP_WAVES, false>;
template <int D>
__device__ __forceinline__ void wide_params_body(const WideJobs& t, const int job, const int blk, float* __restrict__ lds) {
    static_assert(D <= 64, "d = 128 takes wide_params_pair_body");
    using T = WideTile<D>;
    constexpr int T16 = T::T16, S4 = T::S4, LDW = T::LDW, LDG = T::LDG, LDH = T::LDH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = lane & 15, kq = lane >> 4;              // fragment coordinates: row / column index, k index
    const WideLds1<D> s(lds, wave);
    float* const s_red = s.w2;                            // block sums (dW2 [d, d], then the [d, 4] sums)
    const int nblk = t.nblk[job], m = t.m_tgt[job];
    const float* __restrict__ x = t.x[job];
    const float* __restrict__ gout = t.gout[job];
    const float slope = t.slope[job];
    wide_params_stage<D>(s, t, job);
    __syncthreads();
    f32x4w accW[T16][T16];
#pragma unroll
    for (int a = 0; a < T16; ++a)
#pragma unroll
        for (int b = 0; b < T16; ++b) accW[a][b] = f32x4w{0.f, 0.f, 0.f, 0.f};
    float a1acc[T16][4];
#pragma unroll
    for (int a = 0; a < T16; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) a1acc[a][b] = 0.f;

    // the workgroup's contiguous range of target points, dealt over its wavefronts
    const int per = (m + nblk - 1) / nblk;
    const int p0 = blk * per, p1 = p0 + per < m ? p0 + per : m;
    for (int p = p0 + wave; p < p1; p += WP_WAVES) {
        const WideEdge ed = wide_edge(t.idx[job], t.pos_src[job], t.pos_tgt[job], p, e, kq, true);
        // the feature rows and the gradient row are needed behind product (1) only, but depend on nothing but the index row:
        // issued here, they travel while layer 1 and product (1) run
        float xv[T16][4], gi[T16];
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) {
            gi[tj] = gout[(int64_t)p * D + 16 * tj + e];
            wide_x_rows<D>(x, ed, 16 * tj + e, xv[tj]);
        }
        if (kq == 0) s.rel[e] = wide_rel1(ed);
        f32x4w acc[T16];
        wide_product1<D, T16, S4, true>(acc, s.w2, s.a1, ed, slope, 0, e, kq, [&](int k, float h) { s.h[e * LDH + 4 * k + kq] = h; });
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) wide_gh2<D>(s.g, s.coef, acc[tj], gi[tj], xv[tj], ed, 16 * tj + e, kq);
        __builtin_amdgcn_wave_barrier();                         // LDS operations of one wavefront complete in order: tiles are written
        // ---- (3) GW = GH2 W2: A[i = edge][k = c] from the GH2 tile, B[k = c][j = c'] = W2[c][c'].  The d = 32 / 64 form: instruction s
        // holds channels 4 s + kq, the order this pass has summed in since it was written (nothing else forms these widths' products)
#pragma unroll
        for (int tj = 0; tj < T16; ++tj) acc[tj] = f32x4w{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < S4; ++k) {
            const float a = s.g[e * LDG + 4 * k + kq];
#pragma unroll
            for (int tj = 0; tj < T16; ++tj)
                acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s.w2[(4 * k + kq) * LDW + 16 * tj + e], acc[tj], 0, 0, 0);
        }
        // ---- (4) gp = GW lrelu'(H1), [d, 4] sums: acc[tj][r] = GW[edge 4 kq + r][channel c' = 16 tj + e].  The d = 32 / 64 form: float
        // fmaf chains in registers across the wavefront's points (there is room for them here), float64 only over the wavefronts
        {
            float4 rl[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) rl[r] = s.rel[4 * kq + r];
#pragma unroll
            for (int tj = 0; tj < T16; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = s.h[(4 * kq + r) * LDH + 16 * tj + e];
                    const float gp = acc[tj][r] * (h > 0.f ? 1.f : slope);
                    a1acc[tj][0] = fmaf(gp, rl[r].x, a1acc[tj][0]);
                    a1acc[tj][1] = fmaf(gp, rl[r].y, a1acc[tj][1]);
                    a1acc[tj][2] = fmaf(gp, rl[r].z, a1acc[tj][2]);
                    a1acc[tj][3] = fmaf(gp, rl[r].w, a1acc[tj][3]);
                }
        }
        wide_product5<D, T16, 4>(accW, s.g, s.h, 0, e, kq);
        __builtin_amdgcn_wave_barrier();                         // the next point overwrites the tiles
    }
    // ---- block sums.  dW2: the wavefronts add in turn, in rows of d floats (rows of d + 4 measured no faster here: 87.1 against 87.2 us)
    __syncthreads();                                             // every wavefront is done with W2
    wide_dw2_block_sum<D, T16, WP_WAVES, D>(s_red, accW, wave, 0, e, kq);
    wide_store_dw2<D, D>(t.dw2_partial[job] + (int64_t)blk * D * D, s_red);
    __syncthreads();
    // [d, 4] sums: the four k-groups of a wavefront hold different edges of the same channels -> fold over kq by shuffles, then
    // over the wavefronts through LDS in float64
#pragma unroll
    for (int tj = 0; tj < T16; ++tj)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = a1acc[tj][q];
            v += __shfl_xor(v, 16, WAVE);
            v += __shfl_xor(v, 32, WAVE);
            if (kq == 0) s_red[(wave * D + 16 * tj + e) * 4 + q] = v;
        }
    __syncthreads();
    wide_store_a1<D, WP_WAVES>(t.a1_partial[job] + (int64_t)blk * 4 * D, s_red);
}

// d = 128 (the 640-point level): the same pass with a PAIR of wavefronts per target point.  Wavefront `half` of a pair evaluates
// products (1) and (3) for the column tiles 4 half .. 4 half + 3 and product (5) for the row tiles 4 half .. 4 half + 3 (accW: 4 x 8
// tiles = 128 registers).  Both evaluate layer 1 for every k-step (it IS the A fragment of (1)); each stores its half of the H1 tile and
// its columns of the GH2 tile, and the pair reads the other half back from LDS.  Every pair of a workgroup walks the same number of
// points (a pair past the end of the range runs a point with sixteen missing edges: zeros into every sum), so the exchange is a
// workgroup barrier.  The [d, 4] sums of a pair live in LDS, in float64, not in registers (accW leaves none to spare): each wavefront
// adds a point's sums to its channels.  Every product keeps the summation order of the pass it replaces (the dump, crfconv_gemm_jobs,
// the a1 slab pass and the weight-gradient partial pass over the dumped rows), so a training step computes what it computed on that
// path, bit for bit.
template <int D>
using WideLds2 = WideParamsLds<D, WP_PAIRS, true>;
template <int D>
__device__ __forceinline__ void wide_params_pair_body(const WideJobs& t, const int job, const int blk, float* __restrict__ lds) {
    using T = WideTile<D>;
    constexpr int T16 = T::T16, TH = T16 / 2, S4 = T::S4, LDW = T::LDW, LDG = T::LDG, LDH = T::LDH;
    static_assert(T16 % 2 == 0, "tile halves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave >> 1, half = wave & 1;
    const int e = lane & 15, kq = lane >> 4;
    const int t0 = TH * half;                             // this wavefront's first column tile of (1), (3) and row tile of (5)
    const WideLds2<D> s(lds, pair);
    float* const s_red = s.w2;
    double* const my_sum = s.sum + pair * 4 * D;
    const int nblk = t.nblk[job], m = t.m_tgt[job];
    const float* __restrict__ x = t.x[job];
    const float* __restrict__ gout = t.gout[job];
    const float slope = t.slope[job];
    for (int i = threadIdx.x; i < WP_PAIRS * 4 * D; i += WP_BLOCK) s.sum[i] = 0.0;
    wide_params_stage<D>(s, t, job);
    __syncthreads();
    f32x4w accW[TH][T16];
#pragma unroll
    for (int a = 0; a < TH; ++a)
#pragma unroll
        for (int b = 0; b < T16; ++b) accW[a][b] = f32x4w{0.f, 0.f, 0.f, 0.f};

    const int per = (m + nblk - 1) / nblk;
    const int p0 = blk * per, p1 = p0 + per < m ? p0 + per : m;
    for (int pb = p0; pb < p1; pb += WP_PAIRS) {          // the same trip count for every pair: workgroup barriers inside
        const bool active = pb + pair < p1;
        const int p = active ? pb + pair : p0;
        const WideEdge ed = wide_edge(t.idx[job], t.pos_src[job], t.pos_tgt[job], p, e, kq, active);
        if (half == 0 && kq == 0) s.rel[e] = wide_rel1(ed);
        // (1) for this wavefront's column tiles; it stores the H1 channels of its half of the k-steps
        f32x4w acc[TH];
        wide_product1<D, TH, 4, true>(acc, s.w2, s.a1, ed, slope, t0, e, kq, [&](int k, float h) {
            if ((k >= S4 / 2) == (half != 0)) s.h[e * LDH + 4 * k + kq] = h;
        });
#pragma unroll
        for (int tj = 0; tj < TH; ++tj) {
            const int c = 16 * (t0 + tj) + e;
            // (issued ahead of product (1), as the narrower widths do, these rows measured no faster: 121.0 us either way)
            const float gic = gout[(int64_t)p * D + c];
            float xc[4];
            wide_x_rows<D>(x, ed, c, xc);
            wide_gh2<D>(s.g, s.coef, acc[tj], gic, xc, ed, c, kq);
        }
        __syncthreads();                                         // both halves of the pair's GH2, H1 and rel tiles are written
        // ---- (3) GW = GH2 W2 for this wavefront's column tiles (c').  The d = 128 form: the k index of lane group kq in instruction ee
        // of sixteen-channel step k is 16 k + 4 kq + ee -- gemm_tile's order (the product crfconv_gemm_jobs formed from the dumped
        // g_h2), because this pass reproduces the dump + GEMM + a1 passes bit for bit
#pragma unroll
        for (int tj = 0; tj < TH; ++tj) acc[tj] = f32x4w{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int k = 0; k < D / 16; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(s.g + e * LDG + 16 * k + 4 * kq);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int ee = 0; ee < 4; ++ee)
#pragma unroll
                for (int tj = 0; tj < TH; ++tj)
                    acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ee], s.w2[(16 * k + 4 * kq + ee) * LDW + 16 * (t0 + tj) + e], acc[tj], 0, 0, 0);
        }
        // ---- (4) The d = 128 form: gp = GW lrelu'(H1) in float; its products with {rel, 1} and their sums in float64, as a1_reduce_body
        // forms them from the dumped tensors (same reason): over the four rows here, over kq by shuffles, into the pair's LDS sums
        {
            float4 rl[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) rl[r] = s.rel[4 * kq + r];
#pragma unroll
            for (int tj = 0; tj < TH; ++tj) {
                double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = s.h[(4 * kq + r) * LDH + 16 * (t0 + tj) + e];
                    const double gp = (double)(acc[tj][r] * (h > 0.f ? 1.f : slope));
                    v[0] += gp * (double)rl[r].x; v[1] += gp * (double)rl[r].y; v[2] += gp * (double)rl[r].z; v[3] += gp * (double)rl[r].w;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v[c] += __shfl_xor(v[c], 16, WAVE);
                    v[c] += __shfl_xor(v[c], 32, WAVE);
                }
                if (kq == 0) {
                    double* const dst = &my_sum[4 * (16 * (t0 + tj) + e)];
#pragma unroll
                    for (int c = 0; c < 4; ++c) dst[c] += v[c];
                }
            }
        }
        wide_product5<D, TH, 2>(accW, s.g, s.h, t0, e, kq);     // this wavefront's row tiles (c) against every column tile (c')
        __syncthreads();                                         // the next point overwrites the tiles (after the last: everyone is done with W2)
    }
    // ---- block sums.  The two wavefronts of a pair own disjoint rows of dW2; the pairs add in turn, ((p0 + p1) + p2) + p3 -- wgrad_body's
    // order over its four wavefronts, which walk the sixteen-row groups (= points) of a row slice as the pairs walk the points here.
    // Rows of LDW floats: the four k-groups of a wavefront in different banks (7 us of the launch against rows of d floats)
    wide_dw2_block_sum<D, TH, WP_PAIRS, LDW>(s_red, accW, pair, t0, e, kq);
    wide_store_dw2<D, LDW>(t.dw2_partial[job] + (int64_t)blk * D * D, s_red);
    // [d, 4] sums: over the pairs in float64 (every wavefront left s.sum before the loop's last barrier)
    wide_store_a1<D, WP_PAIRS>(t.a1_partial[job] + (int64_t)blk * 4 * D, s.sum);
}

// Every width in ONE launch (round 5: d = 32 and 64; d = 128 since the pair form): the d = 32 layers (854 workgroups at config 2) and
// the d = 64 ones (214) used to be two launches of ~41 us each at the end of the backward pass, neither of which fills the chip; a
// workgroup looks its job up and dispatches on the job's width.  One LDS buffer of the largest width: one workgroup per CU, as the
// d = 64 buffer already meant.
__global__ __launch_bounds__(WP_BLOCK) void wide_params_any_kernel(const WideJobs t) {
    constexpr int LDS_FLOATS = WideLds2<128>::FLOATS;
    static_assert(LDS_FLOATS >= WideLds1<64>::FLOATS && LDS_FLOATS >= WideLds1<32>::FLOATS, "the buffer of the largest width");
    static_assert(LDS_FLOATS * sizeof(float) == 159232, "one workgroup per CU");
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    int job = 0;
    while (job + 1 < t.njobs && t.blk_base[job + 1] <= (int)blockIdx.x) ++job;
    const int blk = (int)blockIdx.x - t.blk_base[job];
    if (t.d[job] == 32) wide_params_body<32>(t, job, blk, lds);
    else if (t.d[job] == 64) wide_params_body<64>(t, job, blk, lds);
    else wide_params_pair_body<128>(t, job, blk, lds);
}

// The d = 128 parameter pass takes the partition of the weight-gradient pass over the m_tgt * 16 dumped edge rows it replaces (wg_plan:
// 256-row slices = 16 points per workgroup, four per pair, at the 640-point level): same slabs, same sums -- dW2 comes out bit-identical
// to the dump + GEMM path's.  The narrower widths: the forward kernels' table (wide_points_per_wave).
static int64_t wide_nblk(int64_t m_tgt, int d) {
    int64_t nb = d == 128 ? wg_plan(m_tgt * 16, 128, 128).nblk : cdiv(m_tgt, wide_points_per_wave(m_tgt) * WP_WAVES);
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    return nb;
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_pointconv_wide_params_supported(int64_t m_tgt, int K, int d) {
    // (d = 128: a pair of wavefronts per point -- one wavefront per point compiles to 256 + 256 registers with a few spilled to scratch,
    // and scratch kernels cannot sit in a replayed hipGraph on ROCm 7.2)
    return (K == 16 && (d == 32 || d == 64 || d == 128) && m_tgt > 0 && m_tgt < ((int64_t)1 << 27)) ? 1 : 0;
}

extern "C" int64_t crfconv_pointconv_wide_params_nblk(int64_t m_tgt, int d) {
    return m_tgt > 0 ? wide_nblk(m_tgt, d) : 0;
}

extern "C" int crfconv_pointconv_wide_params_jobs(const crf_pc_wide_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs || njobs == 0, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(njobs >= 0, CRF_ERR_ARG, "njobs=%d < 0", njobs);
    hipStream_t st = as_stream(stream);
    for (int j = 0; j < njobs; ++j) {
        const crf_pc_wide_job& jb = jobs[j];
        CRF_REQUIRE(crfconv_pointconv_wide_params_supported(jb.m_tgt, jb.K, jb.d) == 1, CRF_ERR_UNSUPPORTED,
                    "job %d: K=%d d=%d m_tgt=%lld outside the matrix-pipe parameter pass (K = 16, d in {32, 64, 128})", j, jb.K, jb.d,
                    (long long)jb.m_tgt);
        CRF_REQUIRE(jb.x && jb.gout && jb.pos_src && jb.pos_tgt && jb.idx32 && jb.A1 && jb.b1 && jb.W2 && jb.ca && jb.cb && jb.cc &&
                        jb.dw2_partial && jb.a1_partial, CRF_ERR_ARG, "job %d: null pointer", j);
    }
    // the jobs in the caller's order, WP_MAX per launch, all widths together (the longest-running width first: its workgroups start first)
    int order[3] = {128, 64, 32};
    int idx[64];
    int nidx = 0;
    for (int w = 0; w < 3; ++w)
        for (int j = 0; j < njobs && nidx < 64; ++j)
            if (jobs[j].d == order[w]) idx[nidx++] = j;
    CRF_REQUIRE(nidx == njobs, CRF_ERR_UNSUPPORTED, "at most 64 jobs per call");
    for (int j0 = 0; j0 < nidx; j0 += WP_MAX) {
        WideJobs t;
        const int n = nidx - j0 < WP_MAX ? nidx - j0 : WP_MAX;
        int64_t blocks = 0;
        for (int k = 0; k < n; ++k) {
            const crf_pc_wide_job& jb = jobs[idx[j0 + k]];
            t.x[k] = jb.x; t.gout[k] = jb.gout; t.pos_src[k] = jb.pos_src; t.pos_tgt[k] = jb.pos_tgt; t.idx[k] = jb.idx32;
            t.A1[k] = jb.A1; t.b1[k] = jb.b1; t.W2[k] = jb.W2; t.ca[k] = jb.ca; t.cb[k] = jb.cb; t.cc[k] = jb.cc;
            t.dw2_partial[k] = jb.dw2_partial; t.a1_partial[k] = jb.a1_partial;
            t.m_tgt[k] = (int)jb.m_tgt; t.nblk[k] = (int)wide_nblk(jb.m_tgt, jb.d); t.slope[k] = jb.slope; t.d[k] = jb.d;
            t.blk_base[k] = (int)blocks;
            blocks += t.nblk[k];
        }
        for (int k = n; k <= WP_MAX; ++k) t.blk_base[k] = (int)blocks;
        for (int k = n; k < WP_MAX; ++k) {
            t.x[k] = t.gout[k] = t.pos_src[k] = t.pos_tgt[k] = t.A1[k] = t.b1[k] = t.W2[k] = t.ca[k] = t.cb[k] = t.cc[k] = nullptr;
            t.idx[k] = nullptr; t.dw2_partial[k] = nullptr; t.a1_partial[k] = nullptr; t.m_tgt[k] = 0; t.nblk[k] = 1; t.slope[k] = 1.f; t.d[k] = 32;
        }
        t.njobs = n;
        hipLaunchKernelGGL(wide_params_any_kernel, dim3((unsigned)blocks), dim3(WP_BLOCK), 0, st, t);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}
