// Backward of the coarse-level MLP block A = lrelu(BN(X W^T), slope) (crfconv_mlp_small_backward*; models/common.py:26-40): row-tile
// partials of the two channel sums of the BatchNorm backward, finished per column slab by its last workgroup (bn_bwd_tile_sums_*),
// then dX = gY W on the tiled product with gY formed while the A operand is loaded (the PRO form of gemm_tile.hpp) -- as two launches
// or as one whose product workgroups wait inside the launch.  Up to 4 independent blocks per call.
#include "gemm_tile.hpp"

namespace crf {

// Row-tile partials of the two channel sums of a BatchNorm backward: partial[tile][0][c] = sum g1, [1][c] = sum g1 yh over the tile's
// BT_ROWS rows (g1 = gA lrelu'(a y + b), yh = (y - mean) rstd).  A workgroup = one tile x 64 channels: 16 lanes x 16 bytes per row
// (whole 256-byte row segments), 16 rows per pass; float32 inside a thread's eight rows, float64 across the 16 row threads.
constexpr int BT_ROWS = 128, BT_CH = 64, BT_NR = BT_ROWS / 16;
// what the LAST workgroup of a column slab leaves for the product launch and the caller
struct TileSumFin {
    unsigned* ticket;          // this slab's ticket word (zero; left zero)
    int ntile;                 // workgroups (row tiles) of the slab
    int training;
    float inv_m;
    float* fin;                // [2][K]
    float* dgamma;             // [K]
    float* dbeta;              // [K]
    unsigned* done = nullptr;  // one-launch form: the job's slab count (GemmPro::sync[0]); `fin` then goes out write-through
};
struct TileSumLds { float red[16][2][64]; int last; };
typedef unsigned int bt_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bn_bwd_tile_sums_body(const float* __restrict__ gA, const float* __restrict__ Y,
                                                       const float* __restrict__ coef, int M, int K, int tile_rows,
                                                       float slope, double* __restrict__ partial, const int bx, const int by,
                                                       const TileSumFin f, TileSumLds& L) {
    float (&s_red)[16][2][64] = L.red;
    int& s_last = L.last;
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = by * BT_CH + 4 * cq;
    const int row0 = bx * tile_rows;
    const int row_end = row0 + tile_rows < M ? row0 + tile_rows : M;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (c < K) {
        const float4 ca = *reinterpret_cast<const float4*>(coef + c), cb = *reinterpret_cast<const float4*>(coef + K + c);
        const float4 mu = *reinterpret_cast<const float4*>(coef + 2 * K + c), rs = *reinterpret_cast<const float4*>(coef + 3 * K + c);
        for (int base = row0; base < row_end; base += BT_ROWS) {      // one trip at <= 3072 rows (tiles of 128 rows)
            float4 g[BT_NR], y[BT_NR];                       // every load of a trip in flight at once: one round trip
#pragma unroll
            for (int u = 0; u < BT_NR; ++u) {
                const int r = base + rl + 16 * u;
                const bool in = r < row_end;
                g[u] = in ? *reinterpret_cast<const float4*>(gA + (int64_t)r * K + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                y[u] = in ? *reinterpret_cast<const float4*>(Y + (int64_t)r * K + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < BT_NR; ++u) {                // (rows past the end hold g = 0: they add nothing)
                float4 v = g[u];
                v.x *= fmaf(ca.x, y[u].x, cb.x) > 0.f ? 1.f : slope;
                v.y *= fmaf(ca.y, y[u].y, cb.y) > 0.f ? 1.f : slope;
                v.z *= fmaf(ca.z, y[u].z, cb.z) > 0.f ? 1.f : slope;
                v.w *= fmaf(ca.w, y[u].w, cb.w) > 0.f ? 1.f : slope;
                s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
                s2.x = fmaf(v.x, (y[u].x - mu.x) * rs.x, s2.x); s2.y = fmaf(v.y, (y[u].y - mu.y) * rs.y, s2.y);
                s2.z = fmaf(v.z, (y[u].z - mu.z) * rs.z, s2.z); s2.w = fmaf(v.w, (y[u].w - mu.w) * rs.w, s2.w);
            }
        }
    }
    *reinterpret_cast<float4*>(&s_red[rl][0][4 * cq]) = s1;
    *reinterpret_cast<float4*>(&s_red[rl][1][4 * cq]) = s2;
    __syncthreads();
    // partial [ntile][2][K] doubles, stored write-through: the slab's last workgroup (another CU, maybe another XCD) reads them
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(partial, f.ntile * 2 * K * 8);
    const int which = threadIdx.x / BT_CH, ch = threadIdx.x - which * BT_CH;
    const bool mine = threadIdx.x < 2 * BT_CH && by * BT_CH + ch < K;
    if (mine) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += (double)s_red[w][which][ch];           // fixed order
        const unsigned long long bits = (unsigned long long)__double_as_longlong(t);
        const bt_u32x2 u = {(unsigned)bits, (unsigned)(bits >> 32)};
        __builtin_amdgcn_raw_buffer_store_b64(u, pr, ((bx * 2 + which) * K + by * BT_CH + ch) * 8, 0, 16);
    }
    // "the last workgroup finishes" (gridsync.hpp), per column slab: its row tiles draw tickets on the slab's word
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(f.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old + 1 == (unsigned)f.ntile;
        if (last) __hip_atomic_store(f.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    if (mine) {
    // the row-tile partials of this thread's (sum, channel) in tile order, all loads of a 24-tile round in flight (one round at <= 3072
    // rows): the order -- hence every bit -- of the sums the product launch used to form per workgroup
    const int cg = by * BT_CH + ch;
    double tot = 0.0;
    for (int t0 = 0; t0 < f.ntile; t0 += 24) {
        double v[24];
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const int tt = t0 + u < f.ntile ? t0 + u : f.ntile - 1;
            const bt_u32x2 w2 = __builtin_amdgcn_raw_buffer_load_b64(pr, ((tt * 2 + which) * K + cg) * 8, 0, 16);
            const double d = __longlong_as_double((long long)(((unsigned long long)w2.y << 32) | w2.x));
            v[u] = t0 + u < f.ntile ? d : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 24; ++u) tot += v[u];
    }
    (which == 0 ? f.dbeta : f.dgamma)[cg] = (float)tot;
    const float mean = f.training ? (float)(tot * (double)f.inv_m) : 0.f;
    if (f.done == nullptr) f.fin[which * K + cg] = mean;
    else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mean), make_rsrc(f.fin, 2 * K * 4), 4 * (which * K + cg), 0, 16);
    }
    if (f.done != nullptr) {                             // the product workgroups of this launch wait for the job's slabs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x < WL_REPL) __hip_atomic_fetch_add(f.done + threadIdx.x * FW_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct TileSumJobs {
    const float* gA[GG_MAX]; const float* Y[GG_MAX]; const float* coef[GG_MAX]; double* partial[GG_MAX];
    float* fin[GG_MAX]; float* dgamma[GG_MAX]; float* dbeta[GG_MAX];
    int M[GG_MAX], K[GG_MAX], tile_rows[GG_MAX], ntile[GG_MAX], training[GG_MAX];
    float slope[GG_MAX], inv_m[GG_MAX];
    unsigned* ticket;          // BT_SLABS lines per job
    int blk_base[GG_MAX + 1];
    int njobs;
};
constexpr int BT_SLABS = GM_PRO_MAXK / BT_CH;      // column slabs of a job at most (8): job j, slab s draws on ticket line 8 j + s
__device__ __forceinline__ void bn_bwd_tile_sums_job(const TileSumJobs& t, const int blk, TileSumLds& L, unsigned* const* done = nullptr) {
    int j = 0;
    while (j + 1 < t.njobs && t.blk_base[j + 1] <= blk) ++j;
    const int local = blk - t.blk_base[j];
    const int ntile = uni(t.ntile[j]);
    const int bx = local % ntile, by = local / ntile;
    TileSumFin f;
    f.ticket = uni(t.ticket) + (j * BT_SLABS + by) * FW_LINE; f.ntile = ntile; f.training = uni(t.training[j]); f.inv_m = uni(t.inv_m[j]);
    f.fin = uni(t.fin[j]); f.dgamma = uni(t.dgamma[j]); f.dbeta = uni(t.dbeta[j]);
    f.done = done != nullptr ? uni(done[j]) : nullptr;
    bn_bwd_tile_sums_body(uni(t.gA[j]), uni(t.Y[j]), uni(t.coef[j]), uni(t.M[j]), uni(t.K[j]), uni(t.tile_rows[j]), uni(t.slope[j]), uni(t.partial[j]),
                          bx, by, f, L);
}
__global__ __launch_bounds__(256) void bn_bwd_tile_sums_jobs_kernel(const TileSumJobs t) {
    __shared__ TileSumLds L;
    bn_bwd_tile_sums_job(t, (int)blockIdx.x, L);
}

// The dX products of the jobs: gY formed on load from (gA, Y) and the finished channel means (the PRO form of gemm_tile.hpp)
struct GemmProJobs {
    const float* A[GG_MAX]; const float* B[GG_MAX]; const float* addend[GG_MAX]; float* C[GG_MAX];
    GemmPro pro[GG_MAX];
    int M[GG_MAX], N[GG_MAX], K[GG_MAX], tiles_x[GG_MAX], wide[GG_MAX];
    int tile_base[GG_MAX + 1];
    int njobs;
};
__global__ __launch_bounds__(GM_BLOCK) void gemm_pro_jobs_kernel(const GemmProJobs t) {
    int j = 0;
    while (j + 1 < t.njobs && t.tile_base[j + 1] <= (int)blockIdx.x) ++j;
    const unsigned local = blockIdx.x - (unsigned)t.tile_base[j];
    GemmPro pro;                                        // the job's entry, pinned into scalar registers
    pro.Y = uni(t.pro[j].Y); pro.coef = uni(t.pro[j].coef); pro.fin = uni(t.pro[j].fin); pro.slope = uni(t.pro[j].slope); pro.gY = uni(t.pro[j].gY);
    pro.mref = uni(t.pro[j].mref); pro.mslope = uni(t.pro[j].mslope);
    const unsigned tx = (unsigned)uni(t.tiles_x[j]);
    const unsigned bx = (unsigned)uni((int)(local % tx)), by = (unsigned)uni((int)(local / tx));
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<1, 2, 2, 2, false, true>()];
    if (uni(t.wide[j]))
        gemm_tile<1, 2, 2, 2, false, true, true, false>(uni(t.A[j]), uni(t.B[j]), nullptr, uni(t.addend[j]), uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]),
                                                        pro, nullptr, bx, by, lds, tx);
    else
        gemm_tile<1, 1, 2, 2, false, true, true, false>(uni(t.A[j]), uni(t.B[j]), nullptr, uni(t.addend[j]), uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]),
                                                        pro, nullptr, bx, by, lds, tx);
}

// BOTH launches of crfconv_mlp_small_backward_jobs as ONE (round 6): workgroups 0 .. nsum - 1 are the tile-sum workgroups, the rest the
// product's.  A product workgroup requests its first operand chunks, then waits until its job's column slabs have left the two channel
// means (GemmPro::sync) -- the tile-sum workgroups have the lower indices, are dispatched first and wait for nobody, so the wait ends
// whatever part of the grid is resident.  What it saves is the launch boundary (drain, cache write-back, dispatch: 4-5 us of stream time
// on launches whose own work is 2-6 us, 21 times per training step).  Same arithmetic in the same order: results are bit-identical to
// the two launches'.
struct SmallBwdSync { unsigned* done[GG_MAX]; int nsum; };
__global__ __launch_bounds__(GM_BLOCK) void mlp_small_bwd_jobs_kernel(const TileSumJobs ts, const GemmProJobs t, const SmallBwdSync sy) {
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<1, 2, 2, 2, false, true>()];
    static_assert(sizeof(TileSumLds) <= sizeof(lds), "the tile-sum workgroups use the product's buffer");
    if ((int)blockIdx.x < sy.nsum) {
        bn_bwd_tile_sums_job(ts, (int)blockIdx.x, *reinterpret_cast<TileSumLds*>(lds), sy.done);
        return;
    }
    const int blk = (int)blockIdx.x - sy.nsum;
    int j = 0;
    while (j + 1 < t.njobs && t.tile_base[j + 1] <= blk) ++j;
    const unsigned local = (unsigned)(blk - t.tile_base[j]);
    GemmPro pro;
    pro.Y = uni(t.pro[j].Y); pro.coef = uni(t.pro[j].coef); pro.fin = uni(t.pro[j].fin); pro.slope = uni(t.pro[j].slope); pro.gY = uni(t.pro[j].gY);
    pro.mref = uni(t.pro[j].mref); pro.mslope = uni(t.pro[j].mslope);
    pro.sync = uni(t.pro[j].sync); pro.need = (unsigned)uni((int)t.pro[j].need); pro.nprod = (unsigned)uni((int)t.pro[j].nprod); pro.fail = uni(t.pro[j].fail);
    const unsigned tx = (unsigned)uni(t.tiles_x[j]);
    const unsigned bx = (unsigned)uni((int)(local % tx)), by = (unsigned)uni((int)(local / tx));
    if (uni(t.wide[j]))
        gemm_tile<1, 2, 2, 2, false, true, true, false>(uni(t.A[j]), uni(t.B[j]), nullptr, uni(t.addend[j]), uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]),
                                                        pro, nullptr, bx, by, lds, tx);
    else
        gemm_tile<1, 1, 2, 2, false, true, true, false>(uni(t.A[j]), uni(t.B[j]), nullptr, uni(t.addend[j]), uni(t.M[j]), uni(t.N[j]), uni(t.K[j]), uni(t.C[j]),
                                                        pro, nullptr, bx, by, lds, tx);
}

}  // namespace crf

extern "C" int crfconv_mlp_small_backward_supported(int64_t M, int Ci, int Co) {
    return (M >= 1 && M < (int64_t)1 << 24 && Ci >= 4 && Co >= 4 && Ci % 4 == 0 && Co % 4 == 0 && Co <= crf::GM_PRO_MAXK) ? 1 : 0;
}

// at most BT_MAXTILES row tiles of 128 rows or proportionally more.  The slab's last workgroup sums them (24 loads in flight per
// round), so the cap trades rounds of that sum against trips of every tile's row loop: 24 tiles was the cap while every workgroup of
// the PRODUCT re-summed them; with the finished means 48 measured 3.836 ms against 3.868 (96 and 192: the same) -- DESIGN 9, T1.
static void bt_plan(int64_t M, int& ntile, int& tile_rows) {
    constexpr int BT_MAXTILES = 48;
    int64_t rows = crf::BT_ROWS;
    if ((M + rows - 1) / rows > BT_MAXTILES) rows = (((M + BT_MAXTILES - 1) / BT_MAXTILES + 15) / 16) * 16;
    tile_rows = (int)rows;
    ntile = (int)((M + rows - 1) / rows);
}

// partials [ntile][2][Co] doubles | the finished means [2][Co] floats (each 256-byte aligned)
static size_t bt_fin_offset(int Co, int ntile) { return (sizeof(double) * 2 * (size_t)Co * (size_t)ntile + 255) & ~(size_t)255; }
extern "C" size_t crfconv_mlp_small_backward_workspace(int64_t M, int Co) {
    if (M < 1 || Co < 1) return 0;
    int ntile, tile_rows;
    bt_plan(M, ntile, tile_rows);
    return bt_fin_offset(Co, ntile) + sizeof(float) * 2 * (size_t)Co + 512;
}

// Backward of one coarse-level MLP block A = lrelu(BN(X W^T), slope) behind its one-launch forward (crfconv_mlp_small_forward),
// in TWO launches: row-tile partials of the channel sums, then dX [M, Ci] = gY W (+ addend) with gY [M, Co] formed in the
// product's operand load (and stored for the weight gradient), dgamma / dbeta on the way.  Same results as
// crfconv_bn_backward followed by crfconv_gemm up to summation order.  coef: the [4][Co] block of the forward.
extern "C" int crfconv_mlp_small_backward(const float* gA, const float* Y, const float* coef, const float* W, const float* addend,
                                          int64_t M, int Ci, int Co, int training, float slope, float* gY, float* dX, float* dgamma,
                                          float* dbeta, void* workspace, size_t workspace_bytes, unsigned* ticket, void* stream) {
    crf_mlp_bwd_job job;
    job.gA = gA; job.Y = Y; job.coef = coef; job.W = W; job.addend = addend; job.M = M; job.Ci = Ci; job.Co = Co; job.training = training;
    job.slope = slope; job.gY = gY; job.dX = dX; job.dgamma = dgamma; job.dbeta = dbeta; job.workspace = workspace; job.workspace_bytes = workspace_bytes;
    job.mask_ref = nullptr; job.mask_slope = 1.f;
    return crfconv_mlp_small_backward_jobs(&job, 1, ticket, stream);
}

// The backward of up to 4 INDEPENDENT coarse-level MLP blocks (crf_mlp_bwd_job: the arguments of crfconv_mlp_small_backward per
// block) in TWO launches for all of them: the row-tile sums of every block, then every block's dX product.  Results per block are
// bit-identical to crfconv_mlp_small_backward's.
static int mlp_small_backward_jobs_impl(const crf_mlp_bwd_job* jobs, int njobs, unsigned* ticket, unsigned* sync_ws, void* stream);
extern "C" int crfconv_mlp_small_backward_jobs(const crf_mlp_bwd_job* jobs, int njobs, unsigned* ticket, void* stream) {
    return mlp_small_backward_jobs_impl(jobs, njobs, ticket, nullptr, stream);
}
// The same as ONE launch (mlp_small_bwd_jobs_kernel): the product's workgroups wait inside the launch for the tile-sum workgroups of
// their job.  sync_ws: the barrier words of crfconv_gridsync_workspace() (zero, left zero; its sticky failure word reports a wait that
// gave up -- that launch's dX / gY are NaN).  Bit-identical results.
extern "C" int crfconv_mlp_small_backward_jobs_one_launch(const crf_mlp_bwd_job* jobs, int njobs, unsigned* ticket, unsigned* sync_ws, void* stream) {
    CRF_REQUIRE(sync_ws != nullptr, CRF_ERR_ARG, "null barrier workspace");
    return mlp_small_backward_jobs_impl(jobs, njobs, ticket, sync_ws, stream);
}
static int mlp_small_backward_jobs_impl(const crf_mlp_bwd_job* jobs, int njobs, unsigned* ticket, unsigned* sync_ws, void* stream) {
    CRF_REQUIRE(jobs && ticket && njobs >= 1 && njobs <= crf::GG_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d) and the ticket words", crf::GG_MAX, njobs);
    crf::TileSumJobs ts{};                              // (slots at or past njobs are never read)
    crf::GemmProJobs gp{};
    crf::SmallBwdSync sy{};
    int64_t blocks = 0, tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        ts.blk_base[j] = (int)blocks;
        gp.tile_base[j] = (int)tiles;
        const crf_mlp_bwd_job& b = jobs[j];
        CRF_REQUIRE(b.gA && b.Y && b.coef && b.W && b.gY && b.dX && b.dgamma && b.dbeta && b.workspace, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(crfconv_mlp_small_backward_supported(b.M, b.Ci, b.Co), CRF_ERR_UNSUPPORTED,
                    "job %d: mlp_small_backward %lld x %d -> %d: widths must be multiples of 4, Co <= %d", j, (long long)b.M, b.Ci, b.Co, crf::GM_PRO_MAXK);
        CRF_REQUIRE(b.workspace_bytes >= crfconv_mlp_small_backward_workspace(b.M, b.Co), CRF_ERR_WORKSPACE, "job %d: workspace too small", j);
        double* partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(b.workspace) + 255) & ~(uintptr_t)255);
        int ntile, tile_rows;
        bt_plan(b.M, ntile, tile_rows);
        ts.gA[j] = b.gA; ts.Y[j] = b.Y; ts.coef[j] = b.coef; ts.partial[j] = partial; ts.M[j] = (int)b.M; ts.K[j] = b.Co; ts.tile_rows[j] = tile_rows;
        float* fin = reinterpret_cast<float*>(reinterpret_cast<char*>(partial) + bt_fin_offset(b.Co, ntile));
        ts.ntile[j] = ntile; ts.slope[j] = b.slope; ts.fin[j] = fin; ts.dgamma[j] = b.dgamma; ts.dbeta[j] = b.dbeta; ts.training[j] = b.training;
        ts.inv_m[j] = (float)(1.0 / (double)b.M);
        blocks += (int64_t)ntile * ((b.Co + crf::BT_CH - 1) / crf::BT_CH);
        crf::GemmPro pro;
        pro.Y = b.Y; pro.coef = b.coef; pro.fin = fin; pro.slope = b.slope; pro.gY = b.gY;
        pro.mref = b.mask_ref; pro.mslope = b.mask_slope;
        gp.A[j] = b.gA; gp.B[j] = b.W; gp.addend[j] = b.addend; gp.C[j] = b.dX; gp.pro[j] = pro; gp.M[j] = (int)b.M; gp.N[j] = b.Ci; gp.K[j] = b.Co;
        crf::GmTilePlan p;
        if (int rc = crf::gm_tile_plan(b.M, b.Ci, true, tiles + blocks, p)) return rc;
        gp.tiles_x[j] = p.tiles_x; gp.wide[j] = p.wide;
        tiles += p.tiles;
        if (sync_ws != nullptr) {                       // the job slot's wait block behind the barrier words
            gp.pro[j].sync = sync_ws + (crf::FW_WAIT + j * crf::WL_LINES) * crf::FW_LINE;
            gp.pro[j].need = (unsigned)((b.Co + crf::BT_CH - 1) / crf::BT_CH);
            gp.pro[j].nprod = (unsigned)p.tiles;
            gp.pro[j].fail = sync_ws + crf::FW_FAIL * crf::FW_LINE;
            sy.done[j] = gp.pro[j].sync;
        }
    }
    ts.njobs = njobs;
    ts.ticket = ticket;
    gp.njobs = njobs;
    hipStream_t st = crf::as_stream(stream);
    if (sync_ws != nullptr) {
        sy.nsum = (int)blocks;
        hipLaunchKernelGGL(crf::mlp_small_bwd_jobs_kernel, dim3((unsigned)(blocks + tiles)), dim3(crf::GM_BLOCK), 0, st, ts, gp, sy);
        CRF_LAUNCH_CHECK();
        return CRF_OK;
    }
    hipLaunchKernelGGL(crf::bn_bwd_tile_sums_jobs_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ts);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(crf::gemm_pro_jobs_kernel, dim3((unsigned)tiles), dim3(crf::GM_BLOCK), 0, st, gp);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
