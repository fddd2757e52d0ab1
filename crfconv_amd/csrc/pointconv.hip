// PointConv, the convolution passes -- the edge kernels whose result is a feature tensor: the eval-mode convolution (forward_kernel),
// the training forward's single pass over the edges (uvstats_kernel, with the CRF matrices riding along: uvstats_hosting_kernel) and
// its element-wise finish (uv_combine_kernel), and the transposed convolution, i.e. the input gradient (bwd_input_kernel, which also
// hosts BatchNorm-2's backward reduction from U and V).  They share ks_sum, and stay in one unit for that reason: with a single caller
// the compiler specialises the helper on its LDS argument and the wide kernels' code changes.
// Semantics, thread mapping and the shared pieces: pointconv_common.hpp.  Passes towards the parameters: pointconv_bwd.hip.
#include "pointconv_common.hpp"
#include "crf_matrices_body.hpp"
#include "uv_fold.hpp"
#include "pointconv_wide.hpp"      // uvstats_mfma_ok / uvstats_mfma_launch: the matrix-pipe statistics pass of the wide layers

namespace crf {

// ------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(PBLOCK) void forward_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ pos_src,
                                                         const float* __restrict__ pos_tgt,
                                                         const int32_t* __restrict__ idx, int K,
                                                         int64_t m_tgt, const float* __restrict__ A1,
                                                         const float* __restrict__ b1,
                                                         const float* __restrict__ W2, float slope,
                                                         const float* __restrict__ a2,
                                                         const float* __restrict__ b2,
                                                         float* __restrict__ out) {
    constexpr int EB = PC<D>::EB;
    __shared__ float4 s_w2t[PC<D>::W2T_F4];
    __shared__ float4 s_scr[PC<D>::SCR_SIZE];
    int lane, wave, q;
    const Row rw = my_row<D>(m_tgt, lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    __syncthreads();
    const float4 sa = ld4(a2 + 4 * q), sb = ld4(b2 + 4 * q);
    const float px = pos_tgt[3 * rw.r], py = pos_tgt[3 * rw.r + 1], pz = pos_tgt[3 * rw.r + 2];
    const int32_t* irow = idx + rw.r * K;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
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
            acc.x = fmaf(fmaf(sa.x, h2[e].x, sb.x), xj[e].x, acc.x);
            acc.y = fmaf(fmaf(sa.y, h2[e].y, sb.y), xj[e].y, acc.y);
            acc.z = fmaf(fmaf(sa.z, h2[e].z, sb.z), xj[e].z, acc.z);
            acc.w = fmaf(fmaf(sa.w, h2[e].w, sb.w), xj[e].w, acc.w);
        }
    }
    __shared__ float4 s_ks[PC<D>::KS > 1 ? PWAVES * WAVE : 1];
    acc = ks_sum<D>(acc, s_ks, lane, wave);
    if (rw.valid && (wave % PC<D>::KS == 0)) st4(out + rw.r * D + 4 * q, acc);
}

// ------------------------------------------------------------------ training forward: one edge pass
// BatchNorm-2 is affine per channel, so the convolution separates:
//   out_i[c] = sum_k (a2 h2_k + b2)[c] x_j[c] = a2[c] U_i[c] + (a2[c] shift[c] + b2[c]) V_i[c],
//   U_i = sum_k (h2_k - shift) * x_j,   V_i = sum_k x_j.
// In training a2 / b2 depend on the batch statistics of h2, which needed an edge pass of their own before the
// convolution pass; this kernel produces U, V AND the statistics partials in ONE pass over the edges, and the
// convolution finishes with an elementwise combine.  U and V also carry everything BatchNorm-2's backward
// needs (sum_e g_w = sum_i g_i V_i,  sum_e g_w (h2 - shift) = sum_i g_i U_i): no edge pass there either.
template <int D>
struct UvLds {
    float4 w2t[PC<D>::W2T_F4];
    float4 scr[PC<D>::SCR_SIZE];
    float red[PWAVES * 2 * D];
    float4 ks[PC<D>::KS > 1 ? PWAVES * WAVE : 1];
    double buf[4 * 256], tot[2 * D];
    int flag;
};
// (bid of n_own: this workgroup among the launch's workgroups that run this body -- all of them, or all but the riders of
// uvstats_hosting_kernel)
template <int D>
__device__ __forceinline__ void uvstats_body(const float* __restrict__ x,
                                                         const float* __restrict__ pos_src,
                                                         const float* __restrict__ pos_tgt,
                                                         const int32_t* __restrict__ idx, int K,
                                                         int64_t m_tgt, const float* __restrict__ A1,
                                                         const float* __restrict__ b1,
                                                         const float* __restrict__ W2, float slope,
                                                         const float* __restrict__ mean_rel,
                                                         float* __restrict__ shift_out,
                                                         float* __restrict__ U, float* __restrict__ V,
                                                         float* __restrict__ partial, unsigned* __restrict__ ticket,
                                                         double* __restrict__ stats, UvLds<D>& L, const unsigned bid, const unsigned n_own) {
    constexpr int EB = PC<D>::EB;
    float4* s_w2t = L.w2t;
    float4* s_scr = L.scr;
    float* sred = L.red;
    int lane, wave, q;
    const unsigned xcd = bid & 7u, base = n_own >> 3, rem = n_own & 7u;                 // xcd_block_id() over the n_own workgroups
    const Row rw = my_row_at<D>(m_tgt, xcd * base + (xcd < rem ? xcd : rem) + (bid >> 3), lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    __syncthreads();
    const float4 shift = mlp.h2_of(mean_rel[0], mean_rel[1], mean_rel[2]);
    if (bid == 0 && threadIdx.x < PC<D>::L) st4(shift_out + 4 * q, shift);

    const float px = pos_tgt[3 * rw.r], py = pos_tgt[3 * rw.r + 1], pz = pos_tgt[3 * rw.r + 2];
    const int32_t* irow = idx + rw.r * K;
    float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if constexpr (EB == 1 && PC<D>::KS == 1) {
        // narrow layers (d <= 16): UG edges per trip -- their index entries, then ALL their feature / position rows, then the
        // arithmetic.  The two-edges-per-trip form below waited on memory 69 % of its cycles at four waves per SIMD
        // (SQ_WAIT_ANY, scratch/run_pcpmc.sh): sixteen dependent load rounds per point, two rows in flight each.
        constexpr int UG = UV_GROUP;
        for (int k0 = 0; k0 < K; k0 += UG) {
            int jj[UG];
#pragma unroll
            for (int e = 0; e < UG; ++e) jj[e] = (k0 + e < K) ? irow[k0 + e] : -1;
            float4 xj[UG];
            float rx[UG], ry[UG], rz[UG];
#pragma unroll
            for (int e = 0; e < UG; ++e) {
                const int64_t j = jj[e] < 0 ? 0 : jj[e];
                xj[e] = ld4(x + j * D + 4 * q);
                rx[e] = px - pos_src[3 * j]; ry[e] = py - pos_src[3 * j + 1]; rz[e] = pz - pos_src[3 * j + 2];
            }
#pragma unroll
            for (int e = 0; e < UG; ++e) {
                const float live = (rw.valid && jj[e] >= 0) ? 1.f : 0.f;
                const float4 xe = jj[e] < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : xj[e];
                float4 pre, h1;
                mlp.layer1(rx[e], ry[e], rz[e], pre, h1);
                const float4 h2 = mlp.layer2(h1);
                const float4 dlt = make_float4((h2.x - shift.x) * live, (h2.y - shift.y) * live, (h2.z - shift.z) * live,
                                               (h2.w - shift.w) * live);
                acc[0].x += dlt.x; acc[0].y += dlt.y; acc[0].z += dlt.z; acc[0].w += dlt.w;
                acc[1] = make_float4(fmaf(dlt.x, dlt.x, acc[1].x), fmaf(dlt.y, dlt.y, acc[1].y),
                                     fmaf(dlt.z, dlt.z, acc[1].z), fmaf(dlt.w, dlt.w, acc[1].w));
                u = make_float4(fmaf(dlt.x, xe.x, u.x), fmaf(dlt.y, xe.y, u.y), fmaf(dlt.z, xe.z, u.z), fmaf(dlt.w, xe.w, u.w));
                v.x += xe.x; v.y += xe.y; v.z += xe.z; v.w += xe.w;
            }
        }
    } else
#pragma unroll 2
    for (int k0 = (wave % PC<D>::KS) * EB; k0 < K; k0 += PC<D>::KS * EB) {
        float4 h1[EB], h2[EB], xj[EB];
        float live[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const int jj = (k0 + e < K) ? irow[k0 + e] : -1;
            const int64_t j = jj < 0 ? 0 : jj;
            live[e] = (rw.valid && jj >= 0) ? 1.f : 0.f;
            xj[e] = ld4(x + j * D + 4 * q);
            if (jj < 0) xj[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 pre;
            mlp.layer1(px - pos_src[3 * j], py - pos_src[3 * j + 1], pz - pos_src[3 * j + 2], pre, h1[e]);
        }
        mlp.layer2_batch(h1, h2, s_scr);
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const float4 dlt = make_float4((h2[e].x - shift.x) * live[e], (h2[e].y - shift.y) * live[e],
                                           (h2[e].z - shift.z) * live[e], (h2[e].w - shift.w) * live[e]);
            acc[0].x += dlt.x; acc[0].y += dlt.y; acc[0].z += dlt.z; acc[0].w += dlt.w;
            acc[1] = make_float4(fmaf(dlt.x, dlt.x, acc[1].x), fmaf(dlt.y, dlt.y, acc[1].y),
                                 fmaf(dlt.z, dlt.z, acc[1].z), fmaf(dlt.w, dlt.w, acc[1].w));
            u = make_float4(fmaf(dlt.x, xj[e].x, u.x), fmaf(dlt.y, xj[e].y, u.y), fmaf(dlt.z, xj[e].z, u.z),
                            fmaf(dlt.w, xj[e].w, u.w));
            v.x += xj[e].x; v.y += xj[e].y; v.z += xj[e].z; v.w += xj[e].w;
        }
    }
    float4* s_ks = L.ks;
    u = ks_sum<D>(u, s_ks, lane, wave);
    v = ks_sum<D>(v, s_ks, lane, wave);
    if (rw.valid && (wave % PC<D>::KS == 0)) {
        st4(U + rw.r * D + 4 * q, u);
        st4(V + rw.r * D + 4 * q, v);
    }
    block_reduce_store<D, 2, true>(acc, sred, partial, lane, wave, q, bid, n_own);
    // with a ticket word the last workgroup to finish sums the rows into stats (reduce_partials_kernel's launch otherwise)
    // (the ticket group comes from bid, this workgroup's number among the n_own -- NOT from blockIdx.x: behind the riders of
    // uvstats_hosting_kernel the two differ, and groups counted on blockIdx.x never fill when n_own % LW_GROUPS != 0)
    if (ticket == nullptr || !last_workgroup_of(ticket, n_own, &L.flag, bid)) return;
    sum_partial_rows_f64<256>(make_rsrc(partial, (int)n_own * 2 * D * 4), (int)n_own, 2 * D, L.buf, L.tot);
    if (threadIdx.x < 2 * D) stats[threadIdx.x] = L.tot[threadIdx.x];
}
template <int D>
__global__ __launch_bounds__(PBLOCK, (D <= 16 ? PC_NARROW_WAVES : 1)) void uvstats_kernel(const float* __restrict__ x, const float* __restrict__ pos_src,
                                                         const float* __restrict__ pos_tgt, const int32_t* __restrict__ idx, int K,
                                                         int64_t m_tgt, const float* __restrict__ A1, const float* __restrict__ b1,
                                                         const float* __restrict__ W2, float slope, const float* __restrict__ mean_rel,
                                                         float* __restrict__ shift_out, float* __restrict__ U, float* __restrict__ V,
                                                         float* __restrict__ partial, unsigned* __restrict__ ticket,
                                                         double* __restrict__ stats) {
    __shared__ UvLds<D> L;
    uvstats_body<D>(x, pos_src, pos_tgt, idx, K, m_tgt, A1, b1, W2, slope, mean_rel, shift_out, U, V, partial, ticket, stats, L, blockIdx.x, gridDim.x);
}
// The same launch CARRYING the CRF layers' matrices (crf_matrices_body.hpp): Q = (I + c^T c)^-1, P = I - Q depend on parameters only,
// yet as a launch of their own (one workgroup per layer, a 27 us chain of 64 dependent pivots) they sat in the middle of the forward's
// launch chain.  Here their workgroups are the FIRST n_side of the grid of the network's first PointConv statistics pass (31 us; four
// workgroups per CU are resident, so only the first ones dispatched are certain to start at once), and nothing waits for them.  The two
// bodies SHARE their LDS (the union below): the riders must not cost the host's workgroups an occupancy step.
#define HOST_PAD(n) (((unsigned)(n) + 7u) & ~7u)
template <int D>
__global__ __launch_bounds__(PBLOCK) void uvstats_hosting_kernel(const float* __restrict__ x, const float* __restrict__ pos_src,
                                                                 const float* __restrict__ pos_tgt, const int32_t* __restrict__ idx, int K,
                                                                 int64_t m_tgt, const float* __restrict__ A1, const float* __restrict__ b1,
                                                                 const float* __restrict__ W2, float slope, const float* __restrict__ mean_rel,
                                                                 float* __restrict__ shift_out, float* __restrict__ U, float* __restrict__ V,
                                                                 float* __restrict__ partial, unsigned* __restrict__ ticket,
                                                                 double* __restrict__ stats, const CrfMatJobs side, const int n_side) {
    static_assert(PBLOCK == CMF_BLOCK, "the riders are workgroups of the host's size");
    __shared__ __attribute__((aligned(16))) union Both { UvLds<D> uv; char mats[CMF_LDS_BYTES]; } L;
    // the riders' slots are padded to a multiple of 8 (HOST_PAD(n_side) workgroups, the surplus ones leave at once): the host's
    // workgroup bid then sits on XCD blockIdx.x % 8 == bid % 8, which is what uvstats_body's XCD-contiguous row order assumes
    const unsigned n_pad = HOST_PAD(n_side);
    if (blockIdx.x < n_pad) {
        const int b = (int)blockIdx.x;
        if (b < n_side) crf_matrices_body(uni(side.c[b]), uni(side.H[b]), uni(side.Q[b]), uni(side.P[b]), L.mats);
        return;
    }
    uvstats_body<D>(x, pos_src, pos_tgt, idx, K, m_tgt, A1, b1, W2, slope, mean_rel, shift_out, U, V, partial, ticket, stats, L.uv,
                    blockIdx.x - n_pad, gridDim.x - n_pad);
}

// out = a2 U + (a2 shift + b2) V   over [m, d] rows (one thread per 4-channel quad).  BatchNorm-2's batch
// coefficients are folded from the statistics right here (a handful of flops per thread, identical in every
// thread of a channel): a2 = gamma rstd, b2 = beta - a2 mean.  Workgroup 0 also publishes a2 / b2 / aux2 = {mean,
// rstd} for the backward kernels and advances the running statistics.
__global__ __launch_bounds__(256) void uv_combine_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                         const double* __restrict__ stats, const float* __restrict__ shift,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         double n_edges, float* __restrict__ run_mean,
                                                         float* __restrict__ run_var, float momentum, float eps,
                                                         int64_t n4, int d4, float* __restrict__ a2_out,
                                                         float* __restrict__ b2_out, double* __restrict__ aux2,
                                                         float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d = 4 * d4;
    const int q = (int)(t % d4);
    float a[4], tv[4];
    const bool publish = blockIdx.x == 0 && threadIdx.x < d4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        const UvCoef k = uv_coef(c, d, stats, shift, gamma, beta, n_edges, eps);      // uv_fold.hpp: shared with the folded consumers
        a[e] = k.a;
        tv[e] = uv_vcoef(k);
        if (publish) uv_publish(c, d, k, n_edges, run_mean, run_var, momentum, a2_out, b2_out, aux2);
    }
    if (t >= n4) return;
    const float4 u = ld4(U + 4 * t), v = ld4(V + 4 * t);
    st4(out + 4 * t, uv_out4(make_float4(a[0], a[1], a[2], a[3]), make_float4(tv[0], tv[1], tv[2], tv[3]), u, v));
}

// ------------------------------------------------------------------ BatchNorm-2 backward from U and V
// partial[blk][0][d] = sum_i g_i V_i, partial[blk][1][d] = sum_i g_i U_i over the block's row slice.
// The LAST workgroup to finish (ticket word, gridsync.hpp) adds the partial rows and derives the coefficients itself: no launch
// behind it.  (ticket == nullptr would leave the rows unsummed; crfconv_pointconv_bwd_input_reduce requires one.)
struct UvRed {                      // arguments of the BatchNorm-2 backward reduction of one PointConv layer (uv_bwd_reduce_body)
    const float* g; const float* U; const float* V;
    long long m;
    int d, nblk;
    float* partial;
    unsigned* ticket;
    const float* shift; const double* aux2; const float* gamma;
    double n_edges;
    int use_batch;
    float* ca; float* cb; float* cc; float* dgamma; float* dbeta;
};
// bid of r.nblk workgroups of 256 threads.  (2 d (256 / (d / 4)) = 2048 floats of LDS whatever d is.)
__device__ __forceinline__ void uv_bwd_reduce_body(const UvRed& r, const unsigned bid) {
    __shared__ float s_uv[2048];                     // [rows per trip][2][d]
    __shared__ double s_buf[4 * 256], s_tot[256];
    __shared__ int s_flag;
    const float* __restrict__ g = r.g; const float* __restrict__ U = r.U; const float* __restrict__ V = r.V;
    const int64_t m = r.m;
    const int d = r.d;
    const int d4 = d >> 2, rpi = 256 / d4;
    const int q = threadIdx.x % d4, rl = threadIdx.x / d4;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    const int64_t stride = (int64_t)r.nblk * rpi;
    auto add = [&](const float4 gg, const float4 uu, const float4 vv) {
        s1 = make_float4(fmaf(gg.x, vv.x, s1.x), fmaf(gg.y, vv.y, s1.y), fmaf(gg.z, vv.z, s1.z), fmaf(gg.w, vv.w, s1.w));
        s2 = make_float4(fmaf(gg.x, uu.x, s2.x), fmaf(gg.y, uu.y, s2.y), fmaf(gg.z, uu.z, s2.z), fmaf(gg.w, uu.w, s2.w));
    };
    int64_t row = (int64_t)bid * rpi + rl;
    for (; row + stride < m; row += 2 * stride) {        // two rows (six 16-byte loads) in flight per thread
        const int64_t o0 = row * d + 4 * q, o1 = (row + stride) * d + 4 * q;
        const float4 g0 = ld4(g + o0), u0 = ld4(U + o0), v0 = ld4(V + o0);
        const float4 g1 = ld4(g + o1), u1 = ld4(U + o1), v1 = ld4(V + o1);
        add(g0, u0, v0);
        add(g1, u1, v1);
    }
    for (; row < m; row += stride) {
        const int64_t o0 = row * d + 4 * q;
        add(ld4(g + o0), ld4(U + o0), ld4(V + o0));
    }
    st4(s_uv + (rl * 2 + 0) * d + 4 * q, s1);
    st4(s_uv + (rl * 2 + 1) * d + 4 * q, s2);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(r.partial, r.nblk * 2 * d * 4);
    for (int t = threadIdx.x; t < 2 * d; t += 256) {
        float a = 0.f;
        for (int i = 0; i < rpi; ++i) a += s_uv[i * 2 * d + t];
        st1_sc1(pr, ((int)bid * 2 * d + t) * 4, a);
    }
    if (r.ticket == nullptr || !last_workgroup_of(r.ticket, (unsigned)r.nblk, &s_flag, bid)) return;
    sum_partial_rows_f64<256>(pr, r.nblk, 2 * d, s_buf, s_tot);
    if ((int)threadIdx.x < d)
        fold2_bwd_coef(threadIdx.x, d, s_tot[threadIdx.x], s_tot[d + threadIdx.x], r.shift, r.aux2, r.gamma, r.n_edges, r.use_batch, r.ca, r.cb, r.cc,
                       r.dgamma, r.dbeta);
}

// ------------------------------------------------------------------ backward: input features
template <int D>
__global__ __launch_bounds__(PBLOCK) void bwd_input_kernel(const float* __restrict__ gout,
                                                           const float* __restrict__ pos_src,
                                                           const float* __restrict__ pos_tgt,
                                                           const int32_t* __restrict__ rev_ptr,
                                                           const int32_t* __restrict__ rev_eid, int K,
                                                           int64_t m_src, const float* __restrict__ A1,
                                                           const float* __restrict__ b1,
                                                           const float* __restrict__ W2, float slope,
                                                           const float* __restrict__ a2,
                                                           const float* __restrict__ b2,
                                                           float* __restrict__ dx, const UvRed red, const int n_own) {
    // round 5: the launch also HOSTS the layer's BatchNorm-2 backward reduction (the workgroups behind the first n_own; red.nblk = 0:
    // none): the two are independent -- dx needs the forward coefficients only -- and the reduction was a launch of its own in front
    // (ten ~8 us launches per step, most of them on grids of a few dozen workgroups)
    if ((int)blockIdx.x >= n_own) {
        uv_bwd_reduce_body(red, blockIdx.x - (unsigned)n_own);
        return;
    }
    constexpr int EB = PC<D>::EB;
    __shared__ float4 s_w2t[PC<D>::W2T_F4];
    __shared__ float4 s_scr[PC<D>::SCR_SIZE];
    int lane, wave, q;
    const unsigned nb = (unsigned)n_own, bb = blockIdx.x;                  // xcd_block_id() of the first n_own workgroups
    const unsigned xcd = bb & 7u, within = bb >> 3, base = nb >> 3, rem = nb & 7u;
    const Row rw = my_row_at<D>(m_src, xcd * base + (xcd < rem ? xcd : rem) + within, lane, wave, q);
    EdgeMLP<D> mlp;
    mlp.init(A1, b1, W2, s_w2t, lane, q, slope);
    __syncthreads();
    const float4 sa = ld4(a2 + 4 * q), sb = ld4(b2 + 4 * q);
    const float sx = pos_src[3 * rw.r], sy = pos_src[3 * rw.r + 1], sz = pos_src[3 * rw.r + 2];
    const int beg = rev_ptr[rw.r];
    const int deg = rw.valid ? rev_ptr[rw.r + 1] - beg : 0;
    int degmax = deg;  // uniform trip count: the MLP exchange needs every lane of a group active
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) degmax = max(degmax, __shfl_xor(degmax, o, WAVE));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // UB edges per trip: their edge ids first, then all their position / gradient rows -- two dependent memory phases per
    // UB edges instead of two per edge (a wavefront iterates to the largest in-degree of its rows, ~35 trips of one edge)
    constexpr int UB = EB > 1 ? EB : 4;
    const int kshift = (K & (K - 1)) == 0 ? __ffs(K) - 1 : -1;
    for (int p0 = (wave % PC<D>::KS) * UB; p0 < degmax; p0 += PC<D>::KS * UB) {
        int eid[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) eid[u] = p0 + u < deg ? rev_eid[beg + p0 + u] : -1;
        float rxs[UB], rys[UB], rzs[UB];
        float4 gs[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            rxs[u] = rys[u] = rzs[u] = 0.f;
            gs[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (eid[u] >= 0) {
                const int64_t i = kshift >= 0 ? (eid[u] >> kshift) : (eid[u] / K);
                rxs[u] = pos_tgt[3 * i] - sx;
                rys[u] = pos_tgt[3 * i + 1] - sy;
                rzs[u] = pos_tgt[3 * i + 2] - sz;
                gs[u] = ld4(gout + i * D + 4 * q);
            }
        }
#pragma unroll
        for (int ub = 0; ub < UB; ub += EB) {
        float4 h1[EB], h2[EB], g[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            g[e] = gs[ub + e];
            float4 pre;
            mlp.layer1(rxs[ub + e], rys[ub + e], rzs[ub + e], pre, h1[e]);
        }
        mlp.layer2_batch(h1, h2, s_scr);
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            acc.x = fmaf(fmaf(sa.x, h2[e].x, sb.x), g[e].x, acc.x);  // g == 0 on inactive slots
            acc.y = fmaf(fmaf(sa.y, h2[e].y, sb.y), g[e].y, acc.y);
            acc.z = fmaf(fmaf(sa.z, h2[e].z, sb.z), g[e].z, acc.z);
            acc.w = fmaf(fmaf(sa.w, h2[e].w, sb.w), g[e].w, acc.w);
        }
        }
    }
    __shared__ float4 s_ks[PC<D>::KS > 1 ? PWAVES * WAVE : 1];
    acc = ks_sum<D>(acc, s_ks, lane, wave);
    if (rw.valid && (wave % PC<D>::KS == 0)) st4(dx + rw.r * D + 4 * q, acc);
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_pointconv_workspace(int64_t m_tgt, int K, int d) {
    if (m_tgt <= 0 || d < 4) return 0;
    const size_t a = (size_t)cdiv(m_tgt, 256) * 9;                               // moments
    const size_t b = (size_t)blocks_for(m_tgt, d) * ((size_t)d * d + 8 * (size_t)d);  // params: float d*d + double 4d
    return sizeof(float) * (a > b ? a : b) + 1024;
}

extern "C" int crfconv_pointconv_forward(const float* x, const float* pos_src, const float* pos_tgt,
                                         const int32_t* idx32, int K, int64_t m_tgt, int d,
                                         const float* A1, const float* b1, const float* W2, float slope,
                                         const float* a2, const float* b2, float* out,
                                         crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(x && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && a2 && b2 && out, CRF_ERR_ARG,
                "null pointer");
    const int64_t nblk = blocks_for(m_tgt, d);
    const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(forward_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(PBLOCK), 0, as_stream(stream), x,
                           pos_src, pos_tgt, idx32, K, m_tgt, A1, b1, W2, slope, a2, b2, out);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_pointconv_forward_uv(const float* x, const float* pos_src, const float* pos_tgt,
                                            const int32_t* idx32, int K, int64_t m_tgt, int d, const float* A1,
                                            const float* b1, const float* W2, float slope, const float* mean_rel3,
                                            float* shift, double* stats, float* U, float* V, void* workspace,
                                            size_t workspace_bytes, unsigned* ticket, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(x && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && mean_rel3 && shift && stats && U && V &&
                    workspace, CRF_ERR_ARG, "null pointer");
    int64_t nblk = blocks_for(m_tgt, d);
    CRF_REQUIRE(workspace_bytes >= sizeof(float) * 2 * d * (size_t)nblk, CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>(workspace);
    if (uvstats_mfma_ok(K, d) && m_tgt < ((int64_t)1 << 27)) {
        // wide layers, K = 16: layer 2 of a point's sixteen edges on the matrix pipe (pointconv_wide_stats.hip)
        const int64_t room = (int64_t)(workspace_bytes / (sizeof(float) * 2 * d));
        if (int rc = uvstats_mfma_launch(x, pos_src, pos_tgt, idx32, m_tgt, d, A1, b1, W2, slope, mean_rel3, shift, U, V, partial, room, &nblk, ticket, stats, st)) return rc;
        return ticket != nullptr ? CRF_OK : reduce_partials(partial, nblk, 2 * d, stats, st);
    }
    if (nblk * (d / 2) > 256 * 24) ticket = nullptr;    // the last workgroup's sum pays up to three rounds of eight 16-byte loads per thread
    const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(uvstats_kernel<decltype(D)::value>, dim3((unsigned)nblk), dim3(PBLOCK), 0, st, x, pos_src, pos_tgt, idx32, K,
                           m_tgt, A1, b1, W2, slope, mean_rel3, shift, U, V, partial, ticket, stats);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return ticket != nullptr ? CRF_OK : reduce_partials(partial, nblk, 2 * d, stats, st);
}

// crfconv_pointconv_forward_uv whose launch also CARRIES crfconv_crf_matrices_batched(c, H, n, Q, P) as its last n workgroups
// (uvstats_hosting_kernel: the riders come first in the grid): for the layer widths crfconv_pointconv_forward_uv_hosts() names -- d = 8, the first PointConv of the
// reference networks (models/point_conv_big.py:107).  Results of both are those of the two separate calls.
extern "C" int crfconv_pointconv_forward_uv_hosts(int K, int d) { return (d == 8 && !uvstats_mfma_ok(K, d)) ? 1 : 0; }
extern "C" int crfconv_pointconv_forward_uv_hosting(const float* x, const float* pos_src, const float* pos_tgt,
                                                    const int32_t* idx32, int K, int64_t m_tgt, int d, const float* A1,
                                                    const float* b1, const float* W2, float slope, const float* mean_rel3,
                                                    float* shift, double* stats, float* U, float* V, void* workspace,
                                                    size_t workspace_bytes, unsigned* ticket, const float* const* c, const int* H,
                                                    int n, float* const* Q, float* const* P, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, K, d)) return rc;
    CRF_REQUIRE(crfconv_pointconv_forward_uv_hosts(K, d) == 1, CRF_ERR_UNSUPPORTED, "forward_uv_hosting: d=%d K=%d is not a hosting width", d, K);
    CRF_REQUIRE(x && pos_src && pos_tgt && idx32 && A1 && b1 && W2 && mean_rel3 && shift && stats && U && V &&
                    workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(c && H && Q && P && n >= 1 && n <= CM_MAX, CRF_ERR_ARG, "null pointer or n=%d outside [1, %d]", n, CM_MAX);
    CrfMatJobs side = {};
    for (int i = 0; i < n; ++i) {
        CRF_REQUIRE(c[i] && Q[i] && P[i] && H[i] >= 1 && H[i] <= 64, CRF_ERR_ARG, "rider %d: null pointer or H=%d outside [1, 64]", i, H[i]);
        side.c[i] = c[i]; side.Q[i] = Q[i]; side.P[i] = P[i]; side.H[i] = H[i];
    }
    const int64_t nblk = blocks_for(m_tgt, d);
    CRF_REQUIRE(workspace_bytes >= sizeof(float) * 2 * d * (size_t)nblk, CRF_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* partial = reinterpret_cast<float*>(workspace);
    if (nblk * (d / 2) > 256 * 24) ticket = nullptr;
    hipLaunchKernelGGL(uvstats_hosting_kernel<8>, dim3((unsigned)nblk + HOST_PAD(n)), dim3(PBLOCK), 0, st, x, pos_src, pos_tgt, idx32, K, m_tgt, A1, b1,
                       W2, slope, mean_rel3, shift, U, V, partial, ticket, stats, side, n);
    CRF_LAUNCH_CHECK();
    return ticket != nullptr ? CRF_OK : reduce_partials(partial, nblk, 2 * d, stats, st);
}

extern "C" int crfconv_pointconv_combine(const float* U, const float* V, const double* stats, const float* shift,
                                         const float* gamma2, const float* beta2, double n_edges, float* run_mean,
                                         float* run_var, float momentum, float eps, int64_t m_tgt, int d, float* a2,
                                         float* b2, double* aux2, float* out, crf_stream_t stream) {
    if (int rc = check_pc(m_tgt, 1, d)) return rc;
    CRF_REQUIRE(U && V && stats && shift && gamma2 && beta2 && a2 && b2 && aux2 && out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE((run_mean == nullptr) == (run_var == nullptr), CRF_ERR_ARG, "running statistics come as a pair");
    const int64_t n4 = m_tgt * (d / 4);
    hipLaunchKernelGGL(uv_combine_kernel, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, as_stream(stream), U, V, stats,
                       shift, gamma2, beta2, n_edges, run_mean, run_var, momentum, eps, n4, d / 4, a2, b2, aux2, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

static int64_t uv_reduce_blocks(int64_t m, int d) {
    const int rpi = 256 / (d / 4);
    const int64_t nb = cdiv(m, (int64_t)rpi * 8);              // ~8 rows per thread
    return nb < 1 ? 1 : (nb > 512 ? 512 : nb);
}

static int uv_red_args(const float* gout, const float* U, const float* V, int64_t m_tgt, int d, const float* shift, const double* aux2,
                       const float* gamma2, double n_edges, int use_batch, float* ca, float* cb, float* cc, float* dgamma2, float* dbeta2,
                       void* workspace, size_t workspace_bytes, unsigned* ticket, UvRed& r) {
    if (int rc = check_pc(m_tgt, 1, d)) return rc;
    CRF_REQUIRE(gout && U && V && shift && aux2 && gamma2 && ca && cb && cc && dgamma2 && dbeta2 && workspace,
                CRF_ERR_ARG, "null pointer");
    const int64_t nblk = uv_reduce_blocks(m_tgt, d);
    CRF_REQUIRE(workspace_bytes >= sizeof(float) * 2 * d * (size_t)nblk, CRF_ERR_WORKSPACE, "workspace too small");
    r.g = gout; r.U = U; r.V = V; r.m = m_tgt; r.d = d; r.nblk = (int)nblk; r.partial = reinterpret_cast<float*>(workspace); r.ticket = ticket;
    r.shift = shift; r.aux2 = aux2; r.gamma = gamma2; r.n_edges = n_edges; r.use_batch = use_batch; r.ca = ca; r.cb = cb; r.cc = cc;
    r.dgamma = dgamma2; r.dbeta = dbeta2;
    return CRF_OK;
}

static int bwd_input_launch(const float* gout, const float* pos_src, const float* pos_tgt, const int32_t* rev_ptr, const int32_t* rev_eid,
                            int K, int64_t m_src, int d, const float* A1, const float* b1, const float* W2, float slope, const float* a2,
                            const float* b2, float* dx, const UvRed& red, crf_stream_t stream) {
    if (int rc = check_pc(m_src, K, d)) return rc;
    CRF_REQUIRE(gout && pos_src && pos_tgt && rev_ptr && rev_eid && A1 && b1 && W2 && a2 && b2 && dx,
                CRF_ERR_ARG, "null pointer");
    const int64_t nblk = blocks_for(m_src, d);
    const bool known = dispatch_width(ALL_WIDTHS, d, [&](auto D) {
        hipLaunchKernelGGL(bwd_input_kernel<decltype(D)::value>, dim3((unsigned)(nblk + red.nblk)), dim3(PBLOCK), 0, as_stream(stream), gout,
                           pos_src, pos_tgt, rev_ptr, rev_eid, K, m_src, A1, b1, W2, slope, a2, b2, dx, red, (int)nblk);
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "d=%d not in {4,8,16,32,64,128}", d);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_pointconv_bwd_input(const float* gout, const float* pos_src, const float* pos_tgt,
                                           const int32_t* rev_ptr, const int32_t* rev_eid, int K,
                                           int64_t m_src, int d, const float* A1, const float* b1,
                                           const float* W2, float slope, const float* a2, const float* b2, float* dx,
                                           crf_stream_t stream) {
    UvRed none{};
    none.nblk = 0;
    return bwd_input_launch(gout, pos_src, pos_tgt, rev_ptr, rev_eid, K, m_src, d, A1, b1, W2, slope, a2, b2, dx, none, stream);
}

// crfconv_pointconv_bwd_input and the layer's BatchNorm-2 backward reduction from U and V (uv_bwd_reduce_body, ticketed) in ONE launch:
// the input gradient needs the forward coefficients only, the reduction's outputs (ca, cb, cc: the parameter pass's; dgamma2, dbeta2)
// are not read before the next launch.
extern "C" int crfconv_pointconv_bwd_input_reduce(const float* gout, const float* pos_src, const float* pos_tgt, const int32_t* rev_ptr,
                                                  const int32_t* rev_eid, int K, int64_t m_src, int64_t m_tgt, int d, const float* A1,
                                                  const float* b1, const float* W2, float slope, const float* a2, const float* b2, float* dx,
                                                  const float* U, const float* V, const float* shift, const double* aux2,
                                                  const float* gamma2, double n_edges, int use_batch, float* ca, float* cb, float* cc,
                                                  float* dgamma2, float* dbeta2, void* workspace, size_t workspace_bytes, unsigned* ticket,
                                                  crf_stream_t stream) {
    CRF_REQUIRE(ticket, CRF_ERR_ARG, "null pointer");
    UvRed r;
    if (int rc = uv_red_args(gout, U, V, m_tgt, d, shift, aux2, gamma2, n_edges, use_batch, ca, cb, cc, dgamma2, dbeta2, workspace,
                             workspace_bytes, ticket, r)) return rc;
    return bwd_input_launch(gout, pos_src, pos_tgt, rev_ptr, rev_eid, K, m_src, d, A1, b1, W2, slope, a2, b2, dx, r, stream);
}
