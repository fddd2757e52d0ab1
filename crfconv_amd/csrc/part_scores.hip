// Part IoU of a ragged batch of shapes (utils/metrics.py:58-112 of the reference, runningScoreShapeNet, for every shape of a batch at once):
// shape s owns rows ptr[s] .. ptr[s + 1], its object category picks a list of part labels out of a CSR table, and its score is the mean
// over that list of (I + eps) / (U + eps), I / U the rows where truth AND / OR prediction equal the label.  Two passes, no float atomics:
//
//   count    ps_rows: one workgroup of PS_TILE = 128 threads per PS_TILE rows of the FLAT batch, so the grid depends on N alone.  The tile's
//            scores -- a contiguous run of rows * C floats that starts on a 16-byte border whenever the tensor does -- are copied to LDS
//            with one float4 per lane (row stride C | 1 there: a thread per row then walks its row without a bank conflict).  The
//            workgroup finds the first shape that reaches into its tile by a binary search of ptr and walks forward; per (tile, shape)
//            segment every thread forms the prediction of its row (the first arg-max over the category's list, or over all C columns),
//            the wavefront counts I, T, P of list entry k with three ballots into lane k, the two wavefronts meet in LDS integer
//            counters, and threads k < len(list) add the non-zero ones onto the [S, 3, C] int32 counters in global memory: integer
//            atomics, 3 len(list) per (tile, shape) at the most.  Integer sums are exact in any order: the same bits in every run.
//   finish   ps_finish: ONE workgroup.  A thread per shape turns the counts into the IEEE double iu_s and flags bad shapes with NaN;
//            after a barrier thread c < n_cat walks the shapes in ascending order and adds those of its category onto cat_sum[c], one
//            float32 rounding per shape (NumPy's `float32_array[c] += python_float`), and counts them.  Every output word has one writer.
//
// The prediction is formed once and serves pred_out and the counts.  ps_rows<.., COUNT = false> is crfconv_part_predict.
#include "common.hpp"

#include "../../include/crfconv_parts.h"

namespace crf {

constexpr int PS_TILE = 128, PS_MAX_LABELS = 64, PS_MAX_CATEGORIES = 64, PS_FINISH_BLOCK = 256;
constexpr int64_t PS_MAX = ((int64_t)1 << 31) - 1;
constexpr double PS_EPS = 1.1920928955078125e-07;          // 2^-23, np.finfo(np.float32).eps

// the part list of category c: `len` labels at parts + begin; len = 0 for a category outside the table
__device__ __forceinline__ int ps_list(const int32_t* __restrict__ parts_ptr, int n_cat, int64_t c, int& begin) {
    begin = 0;
    if (c < 0 || c >= n_cat) return 0;
    const int total = parts_ptr[n_cat];
    begin = parts_ptr[c];
    if (begin < 0 || begin > total) { begin = 0; return 0; }
    int len = parts_ptr[c + 1] - begin;
    len = len > total - begin ? total - begin : len;       // (a broken table: the reads stay inside parts [parts_ptr[n_cat]])
    return len < 0 ? 0 : (len > PS_MAX_LABELS ? PS_MAX_LABELS : len);
}

template <bool SCORES, bool COUNT>
__global__ __launch_bounds__(PS_TILE) void ps_rows_kernel(const int64_t* __restrict__ y_true, const int64_t* __restrict__ y_pred,
                                                          const float* __restrict__ scores, int64_t N, int C, const int64_t* __restrict__ ptr,
                                                          const int64_t* __restrict__ category, int64_t S,
                                                          const int32_t* __restrict__ parts_ptr, const int32_t* __restrict__ parts, int n_cat,
                                                          int restrict_parts, int aligned16, int32_t* __restrict__ counters,
                                                          int64_t* __restrict__ pred_out) {
    extern __shared__ float s_scores[];                    // [rows of the tile][C | 1], SCORES only
    __shared__ int s_cnt[3][PS_MAX_LABELS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int64_t r0 = (int64_t)blockIdx.x * PS_TILE;
    const int64_t r1 = r0 + PS_TILE < N ? r0 + PS_TILE : N;
    const int64_t row = r0 + tid;
    const int stride = C | 1;
    if constexpr (COUNT) {
        if (tid < PS_MAX_LABELS) s_cnt[0][tid] = s_cnt[1][tid] = s_cnt[2][tid] = 0;
    }
    if constexpr (SCORES) {
        const float* __restrict__ src = scores + r0 * C;   // the tile's rows are one contiguous run
        const int n_floats = (int)(r1 - r0) * C;
        const int n_vec = aligned16 ? n_floats >> 2 : 0;   // (r0 C floats = a multiple of 512 bytes: the run starts aligned if scores does)
        for (int i = tid; i < n_vec; i += PS_TILE) {
            const float4 v = ld4(src + 4 * i);
            int r = (4 * i) / C, c = 4 * i - r * C;
            s_scores[r * stride + c] = v.x;
            if (++c == C) { c = 0; ++r; }
            s_scores[r * stride + c] = v.y;
            if (++c == C) { c = 0; ++r; }
            s_scores[r * stride + c] = v.z;
            if (++c == C) { c = 0; ++r; }
            s_scores[r * stride + c] = v.w;
        }
        for (int i = 4 * n_vec + tid; i < n_floats; i += PS_TILE) {
            const int r = i / C;
            s_scores[r * stride + (i - r * C)] = src[i];
        }
    }
    __syncthreads();

    // the first shape whose end lies behind r0; the shapes that meet the tile follow it
    int64_t s = 0;
    {
        int64_t hi = S;
        while (s < hi) {
            const int64_t mid = (s + hi) >> 1;
            if (ptr[mid + 1] > r0) hi = mid;
            else s = mid + 1;
        }
    }
    int t_lab = -1;                                        // the row's true label, -1 when it is outside [0, C)
    if constexpr (COUNT) {
        if (row < r1) {
            const int64_t t = y_true[row];
            t_lab = t >= 0 && t < C ? (int)t : -1;
        }
    }
    int64_t pred = -1;                                     // rows of no shape, and restricted rows of a shape without a list
    for (; s < S; ++s) {
        const int64_t begin = ptr[s];
        if (begin >= r1) break;
        const int64_t end = ptr[s + 1];
        const int64_t lo = begin > r0 ? begin : r0, hi = end < r1 ? end : r1;
        if (lo >= hi) continue;                            // (uniform: every thread reads the same words)
        int list;
        const int len = ps_list(parts_ptr, n_cat, category[s], list);
        const bool mine = row >= lo && row < hi;
        int p_lab = -1;
        if (mine) {
            if constexpr (SCORES) {
                const float* __restrict__ srow = s_scores + tid * stride;
                int arg = -1;
                if (!restrict_parts) {
                    float best = srow[0];
                    arg = 0;
                    for (int c = 1; c < C; ++c) {
                        const float v = srow[c];
                        if (v > best) { best = v; arg = c; }               // strict: the first maximum wins, a NaN never does
                    }
                } else if (len > 0) {
                    arg = parts[list];
                    arg = arg < 0 ? 0 : (arg >= C ? C - 1 : arg);          // (a label outside [0, C): kept inside the row)
                    float best = srow[arg];
                    for (int k = 1; k < len; ++k) {
                        int l = parts[list + k];
                        l = l < 0 ? 0 : (l >= C ? C - 1 : l);
                        const float v = srow[l];
                        if (v > best) { best = v; arg = l; }
                    }
                }
                pred = arg;
                p_lab = arg;
            } else {
                pred = y_pred[row];
                p_lab = pred >= 0 && pred < C ? (int)pred : -1;
            }
        }
        if constexpr (COUNT) {
            // list entry k is counted into lane k: three ballots per entry, no contention
            int c_i = 0, c_t = 0, c_p = 0;
            for (int k = 0; k < len; ++k) {
                const int l = parts[list + k];
                const unsigned long long bt = __ballot(mine && t_lab == l && l >= 0), bp = __ballot(mine && p_lab == l && l >= 0);
                if (lane == k) {
                    c_i = __popcll(bt & bp);
                    c_t = __popcll(bt);
                    c_p = __popcll(bp);
                }
            }
            if (lane < len) {
                if (c_i) atomicAdd(&s_cnt[0][lane], c_i);
                if (c_t) atomicAdd(&s_cnt[1][lane], c_t);
                if (c_p) atomicAdd(&s_cnt[2][lane], c_p);
            }
            __syncthreads();
            if (tid < len) {
                const int l = parts[list + tid];
                if (l >= 0 && l < C) {
                    int32_t* __restrict__ dst = counters + s * 3 * C + l;
                    for (int j = 0; j < 3; ++j) {
                        const int v = s_cnt[j][tid];
                        if (v) atomicAdd(dst + j * C, v);
                    }
                }
                s_cnt[0][tid] = s_cnt[1][tid] = s_cnt[2][tid] = 0;
            }
            __syncthreads();
        }
    }
    if (pred_out && row < r1) pred_out[row] = pred;
}

__global__ __launch_bounds__(PS_FINISH_BLOCK) void ps_finish_kernel(const int32_t* __restrict__ counters, int C, int64_t N,
                                                                    const int64_t* __restrict__ ptr, const int64_t* __restrict__ category,
                                                                    int64_t S, const int32_t* __restrict__ parts_ptr,
                                                                    const int32_t* __restrict__ parts, int n_cat, double* __restrict__ shape_iou,
                                                                    float* __restrict__ cat_sum, int32_t* __restrict__ cat_num,
                                                                    int32_t* __restrict__ bad) {
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int n_bad = 0;
    for (int64_t s = tid; s < S; s += PS_FINISH_BLOCK) {
        const int64_t begin = ptr[s], end = ptr[s + 1], c = category[s];
        int list;
        const int len = ps_list(parts_ptr, n_cat, c, list);
        double iu = __builtin_nan("");
        if (begin >= 0 && begin <= end && end <= N && len > 0) {
            iu = 0.0;
            for (int k = 0; k < len; ++k) {
                const int l = parts[list + k];
                double inter = 0.0, uni_ = 0.0;
                if (l >= 0 && l < C) {
                    const int32_t* __restrict__ src = counters + s * 3 * C + l;
                    const int i = src[0], t = src[C], p = src[2 * C];
                    inter = (double)i;
                    uni_ = (double)(t + p - i);
                }
                iu = dadd_rn(iu, dadd_rn(inter, PS_EPS) / dadd_rn(uni_, PS_EPS));
            }
            iu = iu / (double)len;
        } else {
            ++n_bad;
        }
        shape_iou[s] = iu;
    }
    if (n_bad) atomicAdd(&s_bad, n_bad);
    __syncthreads();                                       // (also orders the shape_iou stores before the reads below: one workgroup)
    if (tid == 0 && s_bad) *bad += s_bad;
    if (tid < n_cat) {
        float sum = cat_sum[tid];
        int num = cat_num[tid];
        for (int64_t s = 0; s < S; ++s) {
            if (category[s] != tid) continue;
            const double iu = shape_iou[s];
            if (iu != iu) continue;                        // a bad shape of this category (its bounds): not accumulated
            sum = (float)dadd_rn((double)sum, iu);         // one float32 rounding per shape
            ++num;
        }
        cat_sum[tid] = sum;
        cat_num[tid] = num;
    }
}

static size_t ps_counter_bytes(int64_t S, int C) { return sizeof(int32_t) * 3 * (size_t)S * (size_t)C; }

static int ps_check_table(const char* who, int64_t N, int C, const int64_t* ptr, const int64_t* category, int64_t S, const int32_t* parts_ptr,
                          const int32_t* parts, int n_cat, int restrict_parts) {
    CRF_REQUIRE(ptr && category && parts_ptr && parts, CRF_ERR_ARG, "%s: null pointer", who);
    CRF_REQUIRE(C >= 1 && C <= PS_MAX_LABELS, CRF_ERR_ARG, "%s: C=%d outside 1..%d", who, C, PS_MAX_LABELS);
    CRF_REQUIRE(n_cat >= 1 && n_cat <= PS_MAX_CATEGORIES, CRF_ERR_ARG, "%s: n_cat=%d outside 1..%d", who, n_cat, PS_MAX_CATEGORIES);
    CRF_REQUIRE(N >= 0 && N <= PS_MAX && S >= 1 && S <= PS_MAX, CRF_ERR_ARG, "%s: N=%lld, S=%lld out of range", who, (long long)N, (long long)S);
    CRF_REQUIRE(restrict_parts == 0 || restrict_parts == 1, CRF_ERR_ARG, "%s: restrict_parts=%d is not 0 or 1", who, restrict_parts);
    return CRF_OK;
}

template <bool SCORES, bool COUNT>
static void ps_launch_rows(const int64_t* y_true, const int64_t* y_pred, const float* scores, int64_t N, int C, const int64_t* ptr,
                           const int64_t* category, int64_t S, const int32_t* parts_ptr, const int32_t* parts, int n_cat, int restrict_parts,
                           int32_t* counters, int64_t* pred_out, hipStream_t st) {
    const size_t lds = SCORES ? sizeof(float) * PS_TILE * (size_t)(C | 1) : 0;             // 33 280 bytes at C = 64
    const int aligned16 = (reinterpret_cast<uintptr_t>(scores) & 15u) == 0;
    hipLaunchKernelGGL((ps_rows_kernel<SCORES, COUNT>), dim3((unsigned)cdiv(N, PS_TILE)), dim3(PS_TILE), lds, st, y_true, y_pred, scores, N, C,
                       ptr, category, S, parts_ptr, parts, n_cat, restrict_parts, aligned16, counters, pred_out);
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_part_scores_workspace(int64_t S, int C) {
    if (S < 1 || S > PS_MAX || C < 1 || C > PS_MAX_LABELS) return 0;
    return ps_counter_bytes(S, C);
}

extern "C" int crfconv_part_scores_update(const int64_t* y_true, const int64_t* y_pred, const float* scores, int64_t N, int C,
                                          const int64_t* ptr, const int64_t* category, int64_t S, const int32_t* parts_ptr,
                                          const int32_t* parts, int n_cat, int restrict_parts, void* workspace, size_t workspace_bytes,
                                          int64_t* pred_out, double* shape_iou, int32_t* counts_out, float* cat_sum, int32_t* cat_num,
                                          int32_t* bad, crf_stream_t stream) {
    const int rc = ps_check_table("part_scores_update", N, C, ptr, category, S, parts_ptr, parts, n_cat, restrict_parts);
    if (rc != CRF_OK) return rc;
    CRF_REQUIRE(shape_iou && cat_sum && cat_num && bad, CRF_ERR_ARG, "part_scores_update: null pointer");
    // (the row arrays of a batch without rows may be NULL: every shape is empty then)
    CRF_REQUIRE(N == 0 || y_true, CRF_ERR_ARG, "part_scores_update: null pointer");
    CRF_REQUIRE(N == 0 || (y_pred != nullptr) != (scores != nullptr), CRF_ERR_ARG,
                "part_scores_update: exactly one of y_pred and scores is given");
    const size_t bytes = ps_counter_bytes(S, C);
    CRF_REQUIRE(counts_out || (workspace && workspace_bytes >= bytes), CRF_ERR_WORKSPACE, "part_scores_update: workspace %zu < %zu",
                workspace ? workspace_bytes : (size_t)0, bytes);
    hipStream_t st = as_stream(stream);
    // the counters ARE counts_out when the caller asks for it: the finish pass has nothing to copy
    int32_t* counters = counts_out ? counts_out : reinterpret_cast<int32_t*>(workspace);
    CRF_HIP(hipMemsetAsync(counters, 0, bytes, st));
    if (N > 0) {
        if (scores)
            ps_launch_rows<true, true>(y_true, nullptr, scores, N, C, ptr, category, S, parts_ptr, parts, n_cat, restrict_parts, counters, pred_out,
                                       st);
        else
            ps_launch_rows<false, true>(y_true, y_pred, nullptr, N, C, ptr, category, S, parts_ptr, parts, n_cat, restrict_parts, counters,
                                        pred_out, st);
        CRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ps_finish_kernel, dim3(1), dim3(PS_FINISH_BLOCK), 0, st, counters, C, N, ptr, category, S, parts_ptr, parts, n_cat,
                       shape_iou, cat_sum, cat_num, bad);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_part_predict(const float* scores, int64_t N, int C, const int64_t* ptr, const int64_t* category, int64_t S,
                                    const int32_t* parts_ptr, const int32_t* parts, int n_cat, int restrict_parts, int64_t* pred_out,
                                    crf_stream_t stream) {
    const int rc = ps_check_table("part_predict", N, C, ptr, category, S, parts_ptr, parts, n_cat, restrict_parts);
    if (rc != CRF_OK) return rc;
    if (N == 0) return CRF_OK;
    CRF_REQUIRE(scores && pred_out, CRF_ERR_ARG, "part_predict: null pointer");
    ps_launch_rows<true, false>(nullptr, nullptr, scores, N, C, ptr, category, S, parts_ptr, parts, n_cat, restrict_parts, nullptr, pred_out,
                                as_stream(stream));
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
