// The per-point Linear layers of the fine levels, forward:  Y = X W^T (+ b)  on the row-streaming fp32 MFMA kernel of
// linear_fwd.hpp, with the optional BatchNorm statistic records, the dropout mask, the column-concatenated operand, the
// eval-mode BatchNorm + activation epilogue and the PointConv combine formed on operand load.  This unit holds the forward
// entry points and instantiates the PRO = false forms of linear_fwd_kernel; the dX product of the fused MLP backward (PRO = true)
// lives in mlp_bwd.hip, the weight gradient in wgrad.hip, BatchNorm from the records in bn_records.hip.
// Also here: the forward job launch of the narrow fine-level blocks (crfconv_linear_forward_jobs) and its form that hosts tiled products.
#include "common.hpp"
#include "linear_fwd.hpp"
#include "gemm_tile.hpp"

using namespace crf;

extern "C" int crfconv_linear_forward_supported(int Ci, int Co) {
    if (Ci < 1 || Co < 1) return 0;
    return lf_lds_bytes(Ci, Co, false) <= 64 * 1024 ? 1 : 0;
}

extern "C" size_t crfconv_linear_forward_stat_records(int64_t M) { return (size_t)crf::lf_blocks(M); }

static int linear_forward_impl(const float* X, const float* Xb, int xsplit, const float* W, const float* bias, int64_t M,
                               int Ci, int Co, int transpose_w, float* Y, float* stat_rec, crf_stream_t stream,
                               LinearDropout drop = LinearDropout(), LinearBnAct bn = LinearBnAct()) {
    CRF_REQUIRE(X && W && Y, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(M > 0, CRF_ERR_ARG, "M must be positive");
    CRF_REQUIRE(crfconv_linear_forward_supported(Ci, Co), CRF_ERR_UNSUPPORTED, "weight slab %dx%d does not fit LDS", Co, Ci);
    CRF_REQUIRE(Xb == nullptr || (xsplit > 0 && xsplit < Ci && xsplit % 4 == 0 && Ci % 4 == 0), CRF_ERR_ARG,
                "two-operand form needs 0 < split < Ci, both multiples of 4 (split=%d Ci=%d)", xsplit, Ci);
    crf::LfArgs a;
    a.X = X; a.W = W; a.bias = bias; a.M = M; a.Ci = Ci; a.Co = Co; a.transpose_w = transpose_w; a.Y = Y; a.stat_partial = stat_rec;
    a.Xb = Xb; a.xsplit = xsplit; a.drop = drop; a.bn = bn;
    return crf::lf_launch<false>(a, bn.coef != nullptr ? crf::EPI_BN_ACT : (drop.counter != nullptr ? crf::EPI_DROPOUT : crf::EPI_NONE), stream);
}

// Y [M, Co] = X [M, Ci] W^T (+ bias);  W is [Co, Ci] row-major, or [Ci, Co] when transpose_w != 0 (the dX product).
// stat_rec (may be NULL): float [records][Co][4] receives per-workgroup {shift, n, sum(y - shift), sum (y - shift)^2}.
extern "C" int crfconv_linear_forward(const float* X, const float* W, const float* bias, int64_t M, int Ci, int Co,
                                      int transpose_w, float* Y, float* stat_rec, crf_stream_t stream) {
    return linear_forward_impl(X, nullptr, 0, W, bias, M, Ci, Co, transpose_w, Y, stat_rec, stream);
}

// crfconv_linear_forward(X, W, NULL, M, Ci, Co, 0, Y, stat_rec) for up to 4 INDEPENDENT layers in ONE launch (linear_fwd_jobs_kernel: the
// jobs' own launches laid end to end -- per job the same workgroups, rows, summation order and records).  The narrow fine-level widths
// only: Ci, Co multiples of 4, Co <= 16, Ci <= 64.
extern "C" int crfconv_linear_forward_jobs_supported(int64_t M, int Ci, int Co) {
    crf::LfArgs a;
    a.M = M; a.Ci = Ci; a.Co = Co;
    return crf::lf_job_ok<false>(a, crf::EPI_NONE) ? 1 : 0;
}

// A job with `tiled` set is crfconv_gemm_stats(X, W, M, Co, Ci, Y, stat_rec) instead -- the block below the row-streaming forms' switch-over
// whose partner is above it (unary_nn / pairwise_nn of the level-1 CRF layer): up to LFS_MAX of them ride as the FIRST workgroups of the
// launch (linear_fwd_jobs_hosting_kernel), each running the 32 x 32 tiles of gm_tile_plan exactly as gemm_stats_jobs_kernel does, on LDS
// carved from the launch's dynamic allocation.  Products of the 32 x 64 tile class (gm_wide) are not taken.
namespace crf {
constexpr int LFS_MAX = 2;
struct LfSideJobs {                                      // (slots at or past n are never read)
    const float* A[LFS_MAX]; const float* B[LFS_MAX]; float* C[LFS_MAX]; float* rec[LFS_MAX];
    int M[LFS_MAX], N[LFS_MAX], K[LFS_MAX], tiles_x[LFS_MAX];
    int tile_base[LFS_MAX + 1];
    int n;
};
static_assert(GM_BLOCK == LF_BLOCK, "the hosted tiles and the row-streaming bodies share one workgroup size");
constexpr size_t LFS_LDS_BYTES = sizeof(float) * gemm_lds_floats<1, 1, 2, 2, true, false>();
__global__ __launch_bounds__(LF_BLOCK) void linear_fwd_jobs_hosting_kernel(const LfJobs t, const LfSideJobs s, const int n_side) {
    if ((int)blockIdx.x < n_side) {
        extern __shared__ __attribute__((aligned(16))) float lf_side_lds[];      // the launch's dynamic LDS: >= LFS_LDS_BYTES
        int j = 0;
        while (j + 1 < s.n && s.tile_base[j + 1] <= (int)blockIdx.x) ++j;
        const unsigned local = blockIdx.x - (unsigned)s.tile_base[j];
        const unsigned tx = (unsigned)uni(s.tiles_x[j]);
        const unsigned bx = (unsigned)uni((int)(local % tx)), by = (unsigned)uni((int)(local / tx));
        gemm_tile<1, 1, 2, 2, true, true, false, true>(uni(s.A[j]), uni(s.B[j]), nullptr, nullptr, uni(s.M[j]), uni(s.N[j]), uni(s.K[j]), uni(s.C[j]), GemmPro(),
                                                       uni(s.rec[j]), bx, by, lf_side_lds);
        return;
    }
    linear_fwd_jobs_block<false>(t, blockIdx.x - (unsigned)n_side);
}
}  // namespace crf

extern "C" int crfconv_linear_forward_jobs_tiled_supported(int64_t M, int Ci, int Co) {
    if (!(M >= 1 && M < ((int64_t)1 << 31) && Co >= 4 && Ci >= 4 && Co % 4 == 0 && Ci % 4 == 0)) return 0;
    return crf::gm_wide(M, Co) ? 0 : 1;
}

extern "C" int crfconv_linear_forward_jobs(const crf_linear_job* jobs, int njobs, crf_stream_t stream) {
    CRF_REQUIRE(jobs && njobs >= 1 && njobs <= crf::LFJ_MAX, CRF_ERR_ARG, "1 .. %d jobs (got %d)", crf::LFJ_MAX, njobs);
    crf::LfArgs a[crf::LFJ_MAX];
    int epi[crf::LFJ_MAX], ns = 0;
    crf::LfSideJobs s{};
    int64_t tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const crf_linear_job& b = jobs[j];
        CRF_REQUIRE(b.X && b.W && b.Y, CRF_ERR_ARG, "job %d: null pointer", j);
        CRF_REQUIRE(b.M > 0, CRF_ERR_ARG, "job %d: M must be positive", j);
        if (b.tiled) {
            const int k = s.n;
            CRF_REQUIRE(ns == 0, CRF_ERR_ARG, "job %d: the tiled jobs come first", j);
            CRF_REQUIRE(k < crf::LFS_MAX, CRF_ERR_UNSUPPORTED, "at most %d tiled jobs", crf::LFS_MAX);
            CRF_REQUIRE(b.stat_rec, CRF_ERR_ARG, "job %d: a tiled job writes statistic records", j);
            CRF_REQUIRE(crfconv_linear_forward_jobs_tiled_supported(b.M, b.Ci, b.Co) == 1, CRF_ERR_UNSUPPORTED,
                        "job %d: tiled %lld x %d -> %d: widths multiples of 4, 32 x 32 tile class", j, (long long)b.M, b.Ci, b.Co);
            crf::GmTilePlan p;
            if (int rc = crf::gm_tile_plan(b.M, b.Co, true, tiles, p)) return rc;
            s.A[k] = b.X; s.B[k] = b.W; s.C[k] = b.Y; s.rec[k] = b.stat_rec; s.M[k] = (int)b.M; s.N[k] = b.Co; s.K[k] = b.Ci;
            s.tiles_x[k] = p.tiles_x;
            s.tile_base[k] = (int)tiles;
            tiles += p.tiles;
            s.n = k + 1;
            continue;
        }
        a[ns].X = b.X; a[ns].W = b.W; a[ns].M = b.M; a[ns].Ci = b.Ci; a[ns].Co = b.Co; a[ns].Y = b.Y; a[ns].stat_partial = b.stat_rec;
        epi[ns++] = crf::EPI_NONE;
    }
    if (s.n == 0) return crf::lf_launch_jobs<false>(a, epi, ns, stream);
    CRF_REQUIRE(ns >= 1, CRF_ERR_UNSUPPORTED, "tiled jobs ride a row-streaming job's launch: none given (crfconv_gemm_stats_jobs takes them alone)");
    for (int k = s.n; k <= crf::LFS_MAX; ++k) s.tile_base[k] = (int)tiles;
    crf::LfJobs t;
    int64_t blocks;
    size_t lds;
    if (int rc = crf::lf_jobs_plan<false>(a, epi, ns, t, blocks, lds)) return rc;
    if (lds < crf::LFS_LDS_BYTES) lds = crf::LFS_LDS_BYTES;
    CRF_REQUIRE(tiles + blocks < ((int64_t)1 << 31), CRF_ERR_UNSUPPORTED, "too many workgroups in one launch");
    hipLaunchKernelGGL(crf::linear_fwd_jobs_hosting_kernel, dim3((unsigned)(tiles + blocks)), dim3(crf::LF_BLOCK), lds, crf::as_stream(stream), t, s,
                       (int)tiles);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

// Y = dropout_mask .* (X W^T or X W) / (1 - p): the input gradient of a Linear that sits BEHIND an nn.Dropout, masked while it
// is written (the mask of crfconv_bn_apply_dropout with the same p, seed and *counter).
extern "C" int crfconv_linear_forward_dropout(const float* X, const float* W, int64_t M, int Ci, int Co, int transpose_w,
                                              float p, uint64_t seed, const int64_t* counter, float* Y, crf_stream_t stream) {
    CRF_REQUIRE(counter, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(p >= 0.f && p < 1.f, CRF_ERR_ARG, "dropout probability %g outside [0, 1)", (double)p);
    LinearDropout d;
    d.counter = reinterpret_cast<const long long*>(counter);
    d.seed = (unsigned long long)seed;
    d.threshold = crf::dropout_threshold(p);
    d.scale = 1.f / (1.f - p);
    return linear_forward_impl(X, nullptr, 0, W, nullptr, M, Ci, Co, transpose_w, Y, nullptr, stream, d);
}

// The same on the column concatenation [Xa | Xb] (Xa [M, split], Xb [M, Ci - split]) without materialising it.
extern "C" int crfconv_linear_forward_cat(const float* Xa, const float* Xb, int split, const float* W, const float* bias,
                                          int64_t M, int Ci, int Co, float* Y, float* stat_rec, crf_stream_t stream) {
    CRF_REQUIRE(Xb, CRF_ERR_ARG, "null pointer");
    return linear_forward_impl(Xa, Xb, split, W, bias, M, Ci, Co, 0, Y, stat_rec, stream);
}

// The eval-mode MLP block as ONE launch: Y = lrelu(add_rn(fmaf(a, [X | Xb] W^T (+ bias), b), skip), slope) with coef = the BatchNorm's
// coefficient rows a | b (crfconv_bn_eval_coef_jobs, crfconv_bn_forward); Xb (with split) and skip may be NULL, slope 1 = no activation.
// Grid, LDS and summation order of crfconv_linear_forward / _cat: bit-identical to that product followed by crfconv_bn_apply
// (and crfconv_add_lrelu with a skip).  Co % 4 == 0.
extern "C" int crfconv_linear_bn_act(const float* X, const float* Xb, int split, const float* W, const float* bias, const float* coef,
                                     const float* skip, float slope, int64_t M, int Ci, int Co, float* Y, crf_stream_t stream) {
    CRF_REQUIRE(coef, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(Co % 4 == 0, CRF_ERR_UNSUPPORTED, "Co=%d must be a multiple of 4", Co);
    LinearBnAct bn;
    bn.coef = coef;
    bn.skip = skip;
    bn.slope = slope;
    return linear_forward_impl(X, Xb, Xb ? split : 0, W, bias, M, Ci, Co, 0, Y, nullptr, stream, LinearDropout(), bn);
}

// crfconv_pointconv_combine + crfconv_linear_forward in ONE launch for lin_out of a fine-level ResNet block: the operand
// out = a2 U + (a2 shift + b2) V is formed while it is loaded (linear_fwd_kernel, EPI_UV) and stored to f->out on the way; a2, b2, aux2
// and BatchNorm-2's running statistics as the combine leaves them.  Only the widths lin_out has at those levels.
extern "C" int crfconv_linear_forward_uv_supported(int Ci, int Co) { return ((Ci == 8 && Co == 32) || (Ci == 16 && Co == 64)) ? 1 : 0; }

extern "C" int crfconv_linear_forward_uv(const crf_uv_fold* f, const float* W, int64_t M, int Ci, int Co, float* Y, float* stat_rec,
                                         crf_stream_t stream) {
    CRF_REQUIRE(W && Y, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(crf::uv_fold_complete(f), CRF_ERR_ARG, "combine record: null pointer, or running statistics not as a pair");
    CRF_REQUIRE(M > 0, CRF_ERR_ARG, "M must be positive");
    CRF_REQUIRE(crfconv_linear_forward_uv_supported(Ci, Co), CRF_ERR_UNSUPPORTED, "combine prologue: %d -> %d is not a fine-level lin_out", Ci, Co);
    const int tco = lf_tco(Ci, Co, false);
    CRF_REQUIRE(16 * tco == Co && lf_hoist_chunks(Ci, true) == 1, CRF_ERR_UNSUPPORTED, "combine prologue: one column group, one chunk");
    crf::LfArgs a;
    a.X = f->U; a.W = W; a.M = M; a.Ci = Ci; a.Co = Co; a.Y = Y; a.stat_partial = stat_rec;
    a.uv = crf::uv_fold_args(f);
    return crf::lf_launch<false>(a, crf::EPI_UV, stream);
}
