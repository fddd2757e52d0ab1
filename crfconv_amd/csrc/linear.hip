// The per-point Linear layers of the fine levels, forward:  Y = X W^T (+ b)  on the row-streaming fp32 MFMA kernel of
// linear_fwd.hpp, with the optional BatchNorm statistic records, the dropout mask, the column-concatenated operand, the
// eval-mode BatchNorm + activation epilogue and the PointConv combine formed on operand load.  This unit holds the forward
// entry points and instantiates the PRO = false forms of linear_fwd_kernel; the dX product of the fused MLP backward (PRO = true)
// lives in mlp_bwd.hip, the weight gradient in wgrad.hip, BatchNorm from the records in bn_records.hip.
#include "common.hpp"
#include "linear_fwd.hpp"

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
