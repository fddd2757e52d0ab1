// What consumes the network's output, on the device so that a training / voting loop
// never leaves it:
//   * confusion matrix of utils/metrics.py:13-27 (runningScore._fast_hist / update), optionally with the arg-max of
//     the logits fused in (trainval.py:108: y_pred.max(dim=1)[1]);
//   * vote accumulator of trainval.py:170-190 (running mean of soft-max probabilities per cloud point) and the
//     re-projection arg-max of trainval.py:198-203.
// Integer / byte work and streaming reductions: HBM-bound, no LDS tiling beyond block-local histograms.
#include "common.hpp"

namespace crf {

constexpr int EV_BLOCK = 256;
constexpr int HIST_LDS_CLASSES = 64;        // n_class^2 uint32 counters in LDS up to this many classes (16 KiB)

__device__ __forceinline__ int argmax_first(const float* __restrict__ row, int C) {
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > best) { best = v; arg = c; }        // strict: first maximum wins, like np.argmax
    }
    return arg;
}

// hist[t * n + p] += 1 for every row whose true label t passes the reference's mask
// (0 <= t < n and t != ignore, metrics.py:14).  pred comes from y_pred or, if logits != NULL, arg-max of the row.
template <bool LDS_HIST>
__global__ __launch_bounds__(EV_BLOCK) void confusion_kernel(const int64_t* __restrict__ y_true,
                                                             const int64_t* __restrict__ y_pred,
                                                             const float* __restrict__ logits, int64_t n_rows, int n,
                                                             int64_t ignore_index, int64_t label_shift,
                                                             unsigned long long* __restrict__ hist,
                                                             int32_t* __restrict__ bad) {
    __shared__ unsigned int s_hist[LDS_HIST ? HIST_LDS_CLASSES * HIST_LDS_CLASSES : 1];
    if constexpr (LDS_HIST) {
        for (int i = threadIdx.x; i < n * n; i += EV_BLOCK) s_hist[i] = 0u;
        __syncthreads();
    }
    int nbad = 0;
    for (int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * EV_BLOCK) {
        const int64_t t = y_true[r] - label_shift;
        if (t < 0 || t >= n || t == ignore_index) continue;
        const int64_t p = logits ? (int64_t)argmax_first(logits + r * n, n) : y_pred[r];
        if (p < 0 || p >= n) { ++nbad; continue; }       // np.bincount would widen the histogram and reshape() fail
        if constexpr (LDS_HIST) atomicAdd(&s_hist[(int)t * n + (int)p], 1u);
        else atomicAdd(&hist[t * n + p], 1ull);
    }
    if (nbad) atomicAdd(bad, nbad);
    if constexpr (LDS_HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < n * n; i += EV_BLOCK)
            if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
    }
}

// one row of the update: dst <- smooth * dst + (1 - smooth) * prob, prob = probs_row or soft-max of logits_row
__device__ __forceinline__ void vote_row(float* __restrict__ dst, const float* __restrict__ probs_row, const float* __restrict__ logits_row,
                                         int C, float smooth, float one_minus) {
    if (logits_row) {
        const float* row = logits_row;
        float mx = row[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
        const float inv = 1.0f / se;
        for (int c = 0; c < C; ++c)
            dst[c] = add_rn(mul_rn(smooth, dst[c]), mul_rn(one_minus, expf(row[c] - mx) * inv));
    } else {
        const float* row = probs_row;
        for (int c = 0; c < C; ++c) dst[c] = add_rn(mul_rn(smooth, dst[c]), mul_rn(one_minus, row[c]));
    }
}

// test_probs[p_idx[r]] = smooth * test_probs[p_idx[r]] + (1 - smooth) * prob[r]   (float32, products and sum each
// rounded once -- numpy evaluates the expression of trainval.py:188 array-op by array-op, so no fused multiply-add).
// prob = probs[r] or soft-max of logits[r].  Rows of one call must be distinct points (a crop is a kNN result).
__global__ __launch_bounds__(EV_BLOCK) void vote_kernel(const float* __restrict__ probs,
                                                        const float* __restrict__ logits,
                                                        const int64_t* __restrict__ point_idx, int64_t n_rows, int C,
                                                        float smooth, float one_minus, float* __restrict__ test_probs,
                                                        int64_t n_cloud, int32_t* __restrict__ bad, int32_t* __restrict__ visits) {
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= n_cloud) { atomicAdd(bad, 1); return; }
    if (visits != nullptr) visits[p] += 1;               // (rows of one call are distinct points: no two threads share p)
    vote_row(test_probs + p * C, probs ? probs + r * C : nullptr, logits ? logits + r * C : nullptr, C, smooth, one_minus);
}

// The same for rows that may name a point more than once (a padded S3DIS crop, s3dis_dataset.py:375-377), with numpy's meaning of
// a[idx] = s * a[idx] + (1 - s) * p (trainval.py:256-262): every right-hand side is formed from the OLD row and of several rows naming
// one point the LAST is stored.  Three passes over the rows, deterministic: (1) integer atomic max of the row number into last[p]
// (-1 everywhere between calls), (2) only row last[p] updates point p and its visit count, (3) last[p] <- -1 again.
__global__ __launch_bounds__(EV_BLOCK) void vote_last_row_kernel(const int64_t* __restrict__ point_idx, int64_t n_rows, int64_t n_cloud,
                                                                 int32_t* __restrict__ last, int32_t* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= n_cloud) { atomicAdd(bad, 1); return; }
    atomicMax(&last[p], (int32_t)r);
}
__global__ __launch_bounds__(EV_BLOCK) void vote_repeated_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                                                 const int64_t* __restrict__ point_idx, int64_t n_rows, int C,
                                                                 float smooth, float one_minus, float* __restrict__ test_probs,
                                                                 int64_t n_cloud, const int32_t* __restrict__ last,
                                                                 int32_t* __restrict__ visits) {
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= n_cloud || last[p] != (int32_t)r) return;
    if (visits != nullptr) visits[p] += 1;               // one row per point passes the test above
    vote_row(test_probs + p * C, probs ? probs + r * C : nullptr, logits ? logits + r * C : nullptr, C, smooth, one_minus);
}
__global__ __launch_bounds__(EV_BLOCK) void vote_last_row_clear_kernel(const int64_t* __restrict__ point_idx, int64_t n_rows,
                                                                       int64_t n_cloud, int32_t* __restrict__ last) {
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p >= 0 && p < n_cloud) last[p] = -1;             // (rows naming one point store the same value)
}

// preds[i] = argmax_c test_probs[proj_idx[i], c] + label_offset   (trainval.py:200-203)
__global__ __launch_bounds__(EV_BLOCK) void project_kernel(const float* __restrict__ test_probs,
                                                           const int64_t* __restrict__ proj_idx, int64_t n_proj, int C,
                                                           int64_t n_cloud, int label_offset,
                                                           uint8_t* __restrict__ preds, int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i >= n_proj) return;
    const int64_t p = proj_idx[i];
    if (p < 0 || p >= n_cloud) { atomicAdd(bad, 1); preds[i] = 0; return; }
    preds[i] = (uint8_t)(argmax_first(test_probs + p * C, C) + label_offset);
}

// ------------------------------------------------------------------------------------------ votes keyed by DEVICE cloud ids
// One sample of a batch: the four kernels above with the cloud looked up on the device (crf_vote_desc table, *cloud_id), so that no
// launch argument depends on which cloud was drawn and the call can sit in a captured graph.  A sample whose cloud id lies outside the
// table is skipped whole and its rows are counted (once: by the first pass of the repeated form).
__device__ __forceinline__ bool vote_cloud(const crf_vote_desc* __restrict__ clouds, int n_clouds, const int64_t* __restrict__ cloud_id,
                                           crf_vote_desc& d) {
    const int64_t c = *cloud_id;
    if (c < 0 || c >= n_clouds) return false;
    d = clouds[c];
    return d.test_probs != nullptr && d.n > 0;
}
__device__ __forceinline__ void vote_count_block(int64_t n_rows, int32_t* __restrict__ bad) {       // every row of a skipped sample, once
    const int64_t first = (int64_t)blockIdx.x * EV_BLOCK;
    if (threadIdx.x == 0 && first < n_rows) atomicAdd(bad, (int32_t)(n_rows - first < EV_BLOCK ? n_rows - first : EV_BLOCK));
}

__global__ __launch_bounds__(EV_BLOCK) void vote_batch_kernel(const crf_vote_desc* __restrict__ clouds, int n_clouds,
                                                              const int64_t* __restrict__ cloud_id, const float* __restrict__ probs,
                                                              const float* __restrict__ logits, const int64_t* __restrict__ point_idx,
                                                              int64_t n_rows, int C, float smooth, float one_minus,
                                                              int32_t* __restrict__ bad) {
    crf_vote_desc d;
    if (!vote_cloud(clouds, n_clouds, cloud_id, d)) { vote_count_block(n_rows, bad); return; }
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= d.n) { atomicAdd(bad, 1); return; }
    if (d.visits != nullptr) d.visits[p] += 1;           // (rows of one sample are distinct points; samples are launches in stream order)
    vote_row(d.test_probs + p * C, probs ? probs + r * C : nullptr, logits ? logits + r * C : nullptr, C, smooth, one_minus);
}

// the repeated form: passes (1) (2) (3) of crfconv_vote_update_repeated; a cloud without a last_row table is skipped like a bad cloud id
__global__ __launch_bounds__(EV_BLOCK) void vote_batch_last_row_kernel(const crf_vote_desc* __restrict__ clouds, int n_clouds,
                                                                       const int64_t* __restrict__ cloud_id,
                                                                       const int64_t* __restrict__ point_idx, int64_t n_rows,
                                                                       int32_t* __restrict__ bad) {
    crf_vote_desc d;
    if (!vote_cloud(clouds, n_clouds, cloud_id, d) || d.last_row == nullptr) { vote_count_block(n_rows, bad); return; }
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= d.n) { atomicAdd(bad, 1); return; }
    atomicMax(&d.last_row[p], (int32_t)r);
}
__global__ __launch_bounds__(EV_BLOCK) void vote_batch_repeated_kernel(const crf_vote_desc* __restrict__ clouds, int n_clouds,
                                                                       const int64_t* __restrict__ cloud_id, const float* __restrict__ probs,
                                                                       const float* __restrict__ logits, const int64_t* __restrict__ point_idx,
                                                                       int64_t n_rows, int C, float smooth, float one_minus) {
    crf_vote_desc d;
    if (!vote_cloud(clouds, n_clouds, cloud_id, d) || d.last_row == nullptr) return;
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p < 0 || p >= d.n || d.last_row[p] != (int32_t)r) return;
    if (d.visits != nullptr) d.visits[p] += 1;           // one row per point passes the test above
    vote_row(d.test_probs + p * C, probs ? probs + r * C : nullptr, logits ? logits + r * C : nullptr, C, smooth, one_minus);
}
__global__ __launch_bounds__(EV_BLOCK) void vote_batch_last_row_clear_kernel(const crf_vote_desc* __restrict__ clouds, int n_clouds,
                                                                             const int64_t* __restrict__ cloud_id,
                                                                             const int64_t* __restrict__ point_idx, int64_t n_rows) {
    crf_vote_desc d;
    if (!vote_cloud(clouds, n_clouds, cloud_id, d) || d.last_row == nullptr) return;
    const int64_t r = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = point_idx[r];
    if (p >= 0 && p < d.n) d.last_row[p] = -1;           // (rows naming one point store the same value)
}

// Confusion matrix straight from a vote table (trainval.py:271-320): row i is compared through p = proj_idx ? proj_idx[i] : i, pred = first
// arg-max of test_probs[p] (an unvoted, all-zero row predicts class 0), t = labels[i] - label_shift; labels outside [0, C) are skipped
// (sklearn's confusion_matrix(labels=...), the mask of utils/metrics.py).  Accumulated like confusion_kernel: exact and order-independent.
template <bool LDS_HIST>
__global__ __launch_bounds__(EV_BLOCK) void vote_confusion_kernel(const float* __restrict__ test_probs, int64_t n_cloud, int C,
                                                                  const int64_t* __restrict__ proj_idx, const int64_t* __restrict__ labels,
                                                                  int64_t n_rows, int64_t label_shift, unsigned long long* __restrict__ hist,
                                                                  int32_t* __restrict__ bad) {
    __shared__ unsigned int s_hist[LDS_HIST ? HIST_LDS_CLASSES * HIST_LDS_CLASSES : 1];
    if constexpr (LDS_HIST) {
        for (int i = threadIdx.x; i < C * C; i += EV_BLOCK) s_hist[i] = 0u;
        __syncthreads();
    }
    int nbad = 0;
    for (int64_t i = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * EV_BLOCK) {
        const int64_t p = proj_idx ? proj_idx[i] : i;
        if (p < 0 || p >= n_cloud) { ++nbad; continue; }
        const int64_t t = labels[i] - label_shift;
        if (t < 0 || t >= C) continue;
        const int pred = argmax_first(test_probs + p * C, C);
        if constexpr (LDS_HIST) atomicAdd(&s_hist[(int)t * C + pred], 1u);
        else atomicAdd(&hist[t * C + pred], 1ull);
    }
    if (nbad) atomicAdd(bad, nbad);
    if constexpr (LDS_HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * C; i += EV_BLOCK)
            if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
    }
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_confusion_accumulate(const int64_t* y_true, const int64_t* y_pred, const float* logits,
                                            int64_t n_rows, int n_class, int64_t ignore_index, int64_t label_shift,
                                            int64_t* hist, int32_t* bad_count, crf_stream_t stream) {
    CRF_REQUIRE(y_true && hist && bad_count && (y_pred || logits), CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n_class >= 1 && n_class <= 4096, CRF_ERR_ARG, "n_class=%d out of range", n_class);
    if (n_rows <= 0) return CRF_OK;
    int64_t blocks = cdiv(n_rows, EV_BLOCK);
    if (blocks > 2048) blocks = 2048;
    auto* h = reinterpret_cast<unsigned long long*>(hist);
    if (n_class <= HIST_LDS_CLASSES)
        hipLaunchKernelGGL(confusion_kernel<true>, dim3((unsigned)blocks), dim3(EV_BLOCK), 0, as_stream(stream), y_true,
                           y_pred, logits, n_rows, n_class, ignore_index, label_shift, h, bad_count);
    else
        hipLaunchKernelGGL(confusion_kernel<false>, dim3((unsigned)blocks), dim3(EV_BLOCK), 0, as_stream(stream), y_true,
                           y_pred, logits, n_rows, n_class, ignore_index, label_shift, h, bad_count);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

static int vote_accumulate_impl(const float* probs, const float* logits, const int64_t* point_idx, int64_t n_rows, int C, double smooth,
                                float* test_probs, int64_t n_cloud, int32_t* bad_count, int32_t* visits, crf_stream_t stream);

extern "C" int crfconv_vote_accumulate(const float* probs, const float* logits, const int64_t* point_idx,
                                       int64_t n_rows, int C, double smooth, float* test_probs, int64_t n_cloud,
                                       int32_t* bad_count, crf_stream_t stream) {
    return vote_accumulate_impl(probs, logits, point_idx, n_rows, C, smooth, test_probs, n_cloud, bad_count, nullptr, stream);
}

// The same, counting the updates of every point in visits [n_cloud] (int32): what crfconv_vote_fold needs to merge tables that
// were accumulated apart (crops of one scene sharded over ranks).
extern "C" int crfconv_vote_accumulate_counted(const float* probs, const float* logits, const int64_t* point_idx,
                                               int64_t n_rows, int C, double smooth, float* test_probs, int64_t n_cloud,
                                               int32_t* bad_count, int32_t* visits, crf_stream_t stream) {
    CRF_REQUIRE(visits, CRF_ERR_ARG, "null pointer");
    return vote_accumulate_impl(probs, logits, point_idx, n_rows, C, smooth, test_probs, n_cloud, bad_count, visits, stream);
}

// acc <- the table that results from applying `later`'s updates AFTER acc's:  a running mean v <- s v + (1 - s) p applied n times
// scales what was there by s^n, so  acc[p] = acc[p] s^later_visits[p] + later[p]  (s^n by n rounded multiplications, as the
// sequential updates round), acc_visits += later_visits.  Merging per-rank tables in rank order gives the table of ONE accumulator
// that saw rank 0's crops first, then rank 1's, ... -- the reference's order-dependent update (trainval.py:188-189) in that order.
__global__ __launch_bounds__(EV_BLOCK) void vote_fold_kernel(float* __restrict__ acc, int32_t* __restrict__ acc_visits,
                                                             const float* __restrict__ later, const int32_t* __restrict__ later_visits,
                                                             int64_t n, int C, float smooth) {
    const int64_t p = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int nv = later_visits[p];
    float d = 1.0f;
    for (int i = 0; i < nv; ++i) d = mul_rn(d, smooth);
    for (int c = 0; c < C; ++c) acc[p * C + c] = add_rn(mul_rn(acc[p * C + c], d), later[p * C + c]);
    acc_visits[p] += nv;
}

extern "C" int crfconv_vote_fold(float* acc, int32_t* acc_visits, const float* later, const int32_t* later_visits, int64_t n, int C,
                                 double smooth, crf_stream_t stream) {
    CRF_REQUIRE(acc && acc_visits && later && later_visits, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(C >= 1 && n >= 0, CRF_ERR_ARG, "C=%d n=%lld invalid", C, (long long)n);
    if (n == 0) return CRF_OK;
    hipLaunchKernelGGL(vote_fold_kernel, dim3((unsigned)cdiv(n, EV_BLOCK)), dim3(EV_BLOCK), 0, as_stream(stream), acc, acc_visits, later,
                       later_visits, n, C, (float)smooth);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

static int vote_accumulate_impl(const float* probs, const float* logits, const int64_t* point_idx, int64_t n_rows, int C, double smooth,
                                float* test_probs, int64_t n_cloud, int32_t* bad_count, int32_t* visits, crf_stream_t stream) {
    CRF_REQUIRE((probs || logits) && point_idx && test_probs && bad_count, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(C >= 1 && n_cloud > 0, CRF_ERR_ARG, "C=%d n_cloud=%lld invalid", C, (long long)n_cloud);
    if (n_rows <= 0) return CRF_OK;
    // (1 - test_smooth) is formed in float64 by the interpreter and rounded when it meets the float32 array
    // both coefficients are python floats (float64) that numpy rounds to float32 when they meet the float32 table
    const float one_minus = (float)(1.0 - smooth);
    hipLaunchKernelGGL(vote_kernel, dim3((unsigned)cdiv(n_rows, EV_BLOCK)), dim3(EV_BLOCK), 0, as_stream(stream), probs,
                       logits, point_idx, n_rows, C, (float)smooth, one_minus, test_probs, n_cloud, bad_count, visits);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_vote_update_repeated(const float* probs, const float* logits, const int64_t* point_idx, int64_t n_rows, int C,
                                            double smooth, float* test_probs, int64_t n_cloud, int32_t* bad_count, int32_t* visits,
                                            int32_t* last_row, crf_stream_t stream) {
    CRF_REQUIRE((probs || logits) && point_idx && test_probs && bad_count && last_row, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(C >= 1 && n_cloud > 0 && n_rows < ((int64_t)1 << 31), CRF_ERR_ARG, "C=%d n_cloud=%lld n_rows=%lld invalid", C,
                (long long)n_cloud, (long long)n_rows);
    if (n_rows <= 0) return CRF_OK;
    const float one_minus = (float)(1.0 - smooth);          // as vote_accumulate_impl
    const dim3 grid((unsigned)cdiv(n_rows, EV_BLOCK)), blk(EV_BLOCK);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(vote_last_row_kernel, grid, blk, 0, st, point_idx, n_rows, n_cloud, last_row, bad_count);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(vote_repeated_kernel, grid, blk, 0, st, probs, logits, point_idx, n_rows, C, (float)smooth, one_minus, test_probs,
                       n_cloud, (const int32_t*)last_row, visits);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(vote_last_row_clear_kernel, grid, blk, 0, st, point_idx, n_rows, n_cloud, last_row);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_vote_project(const float* test_probs, const int64_t* proj_idx, int64_t n_proj, int C,
                                    int64_t n_cloud, int label_offset, uint8_t* preds, int32_t* bad_count,
                                    crf_stream_t stream) {
    CRF_REQUIRE(test_probs && proj_idx && preds && bad_count, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(C >= 1 && C + label_offset <= 256 && n_cloud > 0, CRF_ERR_ARG, "C=%d offset=%d invalid", C, label_offset);
    if (n_proj <= 0) return CRF_OK;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)cdiv(n_proj, EV_BLOCK)), dim3(EV_BLOCK), 0, as_stream(stream),
                       test_probs, proj_idx, n_proj, C, n_cloud, label_offset, preds, bad_count);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_vote_update_batch(const crf_vote_desc* clouds, int n_clouds, const float* probs, const float* logits,
                                         const int64_t* point_idx, const int64_t* cloud_idx, int64_t cloud_idx_stride, int64_t B,
                                         int64_t N, int C, double smooth, int32_t* bad_count, int repeated, crf_stream_t stream) {
    CRF_REQUIRE(clouds && point_idx && cloud_idx && bad_count, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE((probs != nullptr) != (logits != nullptr), CRF_ERR_ARG, "exactly one of probs and logits");
    CRF_REQUIRE(n_clouds >= 1 && C >= 1 && B >= 0 && N >= 0 && N < ((int64_t)1 << 31), CRF_ERR_ARG,
                "n_clouds=%d C=%d B=%lld N=%lld invalid", n_clouds, C, (long long)B, (long long)N);
    if (B == 0 || N == 0) return CRF_OK;
    const float one_minus = (float)(1.0 - smooth);          // as vote_accumulate_impl
    const dim3 grid((unsigned)cdiv(N, EV_BLOCK)), blk(EV_BLOCK);
    hipStream_t st = as_stream(stream);
    // one sample after the other in stream order: the reference's `for b in range(batch_size)`; two samples of one call may name the
    // same cloud and the same points, and the second then sees what the first stored
    for (int64_t b = 0; b < B; ++b) {
        const float* pb = probs ? probs + b * N * C : nullptr;
        const float* lb = logits ? logits + b * N * C : nullptr;
        const int64_t* ib = point_idx + b * N;
        const int64_t* cb = cloud_idx + b * cloud_idx_stride;
        if (repeated) {
            hipLaunchKernelGGL(vote_batch_last_row_kernel, grid, blk, 0, st, clouds, n_clouds, cb, ib, N, bad_count);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(vote_batch_repeated_kernel, grid, blk, 0, st, clouds, n_clouds, cb, pb, lb, ib, N, C, (float)smooth, one_minus);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(vote_batch_last_row_clear_kernel, grid, blk, 0, st, clouds, n_clouds, cb, ib, N);
            CRF_LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(vote_batch_kernel, grid, blk, 0, st, clouds, n_clouds, cb, pb, lb, ib, N, C, (float)smooth, one_minus, bad_count);
            CRF_LAUNCH_CHECK();
        }
    }
    return CRF_OK;
}

extern "C" int crfconv_vote_confusion(const float* test_probs, int64_t n_cloud, int C, const int64_t* proj_idx, const int64_t* labels,
                                      int64_t n_rows, int64_t label_shift, int64_t* hist, int32_t* bad_count, crf_stream_t stream) {
    CRF_REQUIRE(test_probs && labels && hist && bad_count, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(C >= 1 && C <= 4096 && n_cloud > 0, CRF_ERR_ARG, "C=%d n_cloud=%lld invalid", C, (long long)n_cloud);
    CRF_REQUIRE(proj_idx || n_rows <= n_cloud, CRF_ERR_ARG, "n_rows=%lld labels for a cloud of %lld points (no proj_idx)", (long long)n_rows,
                (long long)n_cloud);
    if (n_rows <= 0) return CRF_OK;
    int64_t blocks = cdiv(n_rows, EV_BLOCK);
    if (blocks > 2048) blocks = 2048;
    auto* h = reinterpret_cast<unsigned long long*>(hist);
    if (C <= HIST_LDS_CLASSES)
        hipLaunchKernelGGL(vote_confusion_kernel<true>, dim3((unsigned)blocks), dim3(EV_BLOCK), 0, as_stream(stream), test_probs, n_cloud, C,
                           proj_idx, labels, n_rows, label_shift, h, bad_count);
    else
        hipLaunchKernelGGL(vote_confusion_kernel<false>, dim3((unsigned)blocks), dim3(EV_BLOCK), 0, as_stream(stream), test_probs, n_cloud, C,
                           proj_idx, labels, n_rows, label_shift, h, bad_count);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
