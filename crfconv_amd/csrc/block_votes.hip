// Per-block scores merged back onto the points of the scenes: the inverse of the sliding block split (blocks.hip).  A point lies in up
// to 64 blocks (checked in sliding_blocks); the networks return one row of scores per block ROW, and the merge is a sum over a point's
// rows.  Scattering the rows onto the points would need float atomics -- the order of the adds, and so the bits, would change from run
// to run -- so the POINT gathers its rows instead, through an inverse table built once per split:
//
//   reverse   bv_keys (key = rows[r], value = r | core flag << 31) | rsort_pairs_u64 over the bytes N - 1 needs: stable, so the rows of
//             a point ascend | bv_lists: every sorted item writes the rev_ptr entries between its predecessor's key and its own (the
//             last one also those up to N) and its value: no atomics, every word has one writer
//   update    bv_update: one thread per (point, class).  A workgroup takes G = 256 / C whole points, thread t is class t % C of point
//             t / C: the lanes of a point read the same list entries (one request) and neighbouring floats of a score row.  The sum
//             runs in ascending row order with singly rounded adds; sums and count are read and written by their one owner.
//   result    bv_result: the same mapping writes sums or sums / count; the thread of class 0 walks the C sums for the first arg-max.
//
// The core flag rides in bit 31 of a list entry (R < 2^31), so the update never gathers mask.  'prefer' -- core rows if the point has
// one anywhere in the split -- is decided over the point's WHOLE list, also when the scores cover a part of the rows: a chunked run and
// a one-shot run use the same rows.
#include "common.hpp"

#include "../../include/crfconv_block_votes.h"
#include "radix_sort.hpp"

namespace crf {

enum { BV_ALL = 0, BV_ONLY = 1, BV_PREFER = 2 };
constexpr uint32_t BV_CORE = 0x80000000u;
constexpr int BV_MAX_CLASSES = 64, BV_BLOCK = 256;
constexpr int64_t BV_MAX = ((int64_t)1 << 31) - 1;

__global__ __launch_bounds__(256) void bv_keys_kernel(const int64_t* __restrict__ rows, const int8_t* __restrict__ mask, int64_t R, int64_t N,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    int64_t p = rows[r];
    p = p < 0 ? 0 : (p >= N ? N - 1 : p);                  // (a row outside the points: kept inside, so bv_lists stays inside rev_ptr)
    keys[r] = (unsigned long long)p;
    vals[r] = (uint32_t)r | (mask[r] != 0 ? BV_CORE : 0u);
}

// sorted item i starts the list of every point in (keys[i - 1], keys[i]]: the points in between have no row and an empty list
__global__ __launch_bounds__(256) void bv_lists_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t R,
                                                       int64_t N, int64_t* __restrict__ rev_ptr, int32_t* __restrict__ rev_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    int64_t k = (int64_t)keys[i];
    k = k >= N ? N - 1 : k;                                // (cannot happen: bv_keys wrote them)
    const int64_t prev = i ? (int64_t)keys[i - 1] : -1;
    for (int64_t q = prev + 1; q <= k; ++q) rev_ptr[q] = i;
    if (i == R - 1)
        for (int64_t q = k + 1; q <= N; ++q) rev_ptr[q] = R;
    rev_rows[i] = (int32_t)vals[i];
}

// One thread per (point, class); G points per workgroup, G * C <= 256 threads at work.
template <bool EXP>
__global__ __launch_bounds__(BV_BLOCK) void bv_update_kernel(const float* __restrict__ scores, int64_t R_part, int64_t row_offset, int C, int G,
                                                             const int64_t* __restrict__ rev_ptr, const int32_t* __restrict__ rev_rows,
                                                             int64_t R, int64_t N, int core, float* __restrict__ sums,
                                                             int32_t* __restrict__ count) {
    const int t = threadIdx.x;
    if (t >= G * C) return;
    const int dp = t / C, c = t - dp * C;
    const int64_t p = (int64_t)blockIdx.x * G + dp;
    if (p >= N) return;
    int64_t lo = rev_ptr[p], hi = rev_ptr[p + 1];
    lo = lo < 0 ? 0 : (lo > R ? R : lo);
    hi = hi < lo ? lo : (hi > R ? R : hi);
    float s_all = 0.f, s_core = 0.f;
    int n_all = 0, n_core = 0;
    bool any_core = false;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t v = (uint32_t)rev_rows[i];
        const bool is_core = (v & BV_CORE) != 0u;
        any_core |= is_core;
        const int64_t q = (int64_t)(v & ~BV_CORE) - row_offset;
        if (q >= R_part && (core != BV_PREFER || any_core)) break;          // rows ascend: nothing further lies in the range
        if (q < 0 || q >= R_part) continue;
        float term = scores[q * C + c];
        if constexpr (EXP) term = expf(term);
        s_all = n_all ? add_rn(s_all, term) : term;
        ++n_all;
        if (is_core) {
            s_core = n_core ? add_rn(s_core, term) : term;
            ++n_core;
        }
    }
    const bool use_core = core == BV_ONLY || (core == BV_PREFER && any_core);
    const float s = use_core ? s_core : s_all;
    const int n = use_core ? n_core : n_all;
    if (n == 0) return;
    sums[p * C + c] = add_rn(sums[p * C + c], s);
    if (c == 0) count[p] += n;
}

template <bool MEAN>
__global__ __launch_bounds__(BV_BLOCK) void bv_result_kernel(const float* __restrict__ sums, const int32_t* __restrict__ count, int64_t N, int C,
                                                             int G, int64_t fill, float* __restrict__ out, int64_t* __restrict__ pred) {
    const int t = threadIdx.x;
    if (t >= G * C) return;
    const int dp = t / C, c = t - dp * C;
    const int64_t p = (int64_t)blockIdx.x * G + dp;
    if (p >= N) return;
    const int n = count[p];
    const float* row = sums + p * C;
    float v = 0.f;
    if (n != 0) {
        v = row[c];
        if constexpr (MEAN) v = __fdiv_rn(v, (float)n);
    }
    out[p * C + c] = v;
    if (c != 0) return;
    int64_t arg = fill;
    if (n != 0) {
        float best = row[0];
        arg = 0;
        for (int k = 1; k < C; ++k) {
            const float u = row[k];
            if (u > best) { best = u; arg = k; }           // strict: the first maximum wins, as argmax_first of evaluate.hip
        }
    }
    pred[p] = arg;
}

static size_t bv_al(size_t v) { return (v + 255) & ~(size_t)255; }

struct BvLayout { size_t keys_a, keys_b, vals_a, vals_b, temp, total; };
static BvLayout bv_layout(int64_t R) {
    BvLayout L;
    size_t o = 0;
    L.keys_a = o; o += bv_al(sizeof(unsigned long long) * (size_t)R);
    L.keys_b = o; o += bv_al(sizeof(unsigned long long) * (size_t)R);
    L.vals_a = o; o += bv_al(sizeof(uint32_t) * (size_t)R);
    L.vals_b = o; o += bv_al(sizeof(uint32_t) * (size_t)R);
    L.temp = o;   o += bv_al(rsort_workspace(R));
    L.total = o + 256;
    return L;
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_block_reverse_workspace(int64_t N, int64_t R) {
    if (N < 1 || N > BV_MAX || R < 1 || R > BV_MAX) return 0;
    return bv_layout(R).total;
}

extern "C" int crfconv_block_reverse(const int64_t* rows, int64_t R, int64_t N, const int8_t* mask, void* workspace, size_t workspace_bytes,
                                     int64_t* rev_ptr, int32_t* rev_rows, crf_stream_t stream) {
    CRF_REQUIRE(rows && mask && workspace && rev_ptr && rev_rows, CRF_ERR_ARG, "block_reverse: null pointer");
    CRF_REQUIRE(N >= 1 && N <= BV_MAX && R >= 1 && R <= BV_MAX, CRF_ERR_ARG, "block_reverse: N=%lld, R=%lld out of range", (long long)N,
                (long long)R);
    const BvLayout L = bv_layout(R);
    CRF_REQUIRE(workspace_bytes >= L.total, CRF_ERR_WORKSPACE, "block_reverse: workspace %zu < %zu", workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    auto* keys_a = reinterpret_cast<unsigned long long*>(ws + L.keys_a);
    auto* keys_b = reinterpret_cast<unsigned long long*>(ws + L.keys_b);
    uint32_t* vals_a = reinterpret_cast<uint32_t*>(ws + L.vals_a);
    uint32_t* vals_b = reinterpret_cast<uint32_t*>(ws + L.vals_b);
    const dim3 blk(256), per_row((unsigned)cdiv(R, 256));
    hipLaunchKernelGGL(bv_keys_kernel, per_row, blk, 0, st, rows, mask, R, N, keys_a, vals_a);
    CRF_LAUNCH_CHECK();
    int bits = 0;                                          // of the largest point number
    while (bits < 64 && ((unsigned long long)(N - 1) >> bits) != 0ull) ++bits;
    const int where = rsort_pairs_u64(keys_a, vals_a, keys_b, vals_b, R, 0, 8 * ((bits + 7) / 8), ws + L.temp, st);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(bv_lists_kernel, per_row, blk, 0, st, where ? keys_b : keys_a, where ? vals_b : vals_a, R, N, rev_ptr, rev_rows);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_block_votes_update(const float* scores, int64_t R_part, int64_t row_offset, int C, const int64_t* rev_ptr,
                                          const int32_t* rev_rows, int64_t R, int64_t N, int core, int use_exp, float* sums, int32_t* count,
                                          crf_stream_t stream) {
    CRF_REQUIRE(scores && rev_ptr && rev_rows && sums && count, CRF_ERR_ARG, "block_votes_update: null pointer");
    CRF_REQUIRE(C >= 1 && C <= BV_MAX_CLASSES, CRF_ERR_ARG, "block_votes_update: C=%d outside 1..%d", C, BV_MAX_CLASSES);
    CRF_REQUIRE(N >= 1 && N <= BV_MAX && R >= 1 && R <= BV_MAX, CRF_ERR_ARG, "block_votes_update: N=%lld, R=%lld out of range", (long long)N,
                (long long)R);
    CRF_REQUIRE(R_part >= 0 && row_offset >= 0 && row_offset <= R && R_part <= R - row_offset, CRF_ERR_ARG,
                "block_votes_update: rows %lld .. %lld + %lld outside 0 .. %lld", (long long)row_offset, (long long)row_offset, (long long)R_part,
                (long long)R);
    CRF_REQUIRE(core == BV_ALL || core == BV_ONLY || core == BV_PREFER, CRF_ERR_ARG, "block_votes_update: core=%d is not 0, 1 or 2", core);
    CRF_REQUIRE(use_exp == 0 || use_exp == 1, CRF_ERR_ARG, "block_votes_update: use_exp=%d is not 0 or 1", use_exp);
    if (R_part == 0) return CRF_OK;
    const int G = BV_BLOCK / C;
    const dim3 grid((unsigned)cdiv(N, G)), blk(BV_BLOCK);
    hipStream_t st = as_stream(stream);
    if (use_exp)
        hipLaunchKernelGGL(bv_update_kernel<true>, grid, blk, 0, st, scores, R_part, row_offset, C, G, rev_ptr, rev_rows, R, N, core, sums, count);
    else
        hipLaunchKernelGGL(bv_update_kernel<false>, grid, blk, 0, st, scores, R_part, row_offset, C, G, rev_ptr, rev_rows, R, N, core, sums, count);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_block_votes_result(const float* sums, const int32_t* count, int64_t N, int C, int reduce, int64_t fill, float* scores_out,
                                          int64_t* pred, crf_stream_t stream) {
    CRF_REQUIRE(sums && count && scores_out && pred, CRF_ERR_ARG, "block_votes_result: null pointer");
    CRF_REQUIRE(C >= 1 && C <= BV_MAX_CLASSES, CRF_ERR_ARG, "block_votes_result: C=%d outside 1..%d", C, BV_MAX_CLASSES);
    CRF_REQUIRE(N >= 1 && N <= BV_MAX, CRF_ERR_ARG, "block_votes_result: N=%lld out of range", (long long)N);
    CRF_REQUIRE(reduce == 0 || reduce == 1, CRF_ERR_ARG, "block_votes_result: reduce=%d is not 0 (sum) or 1 (mean)", reduce);
    const int G = BV_BLOCK / C;
    const dim3 grid((unsigned)cdiv(N, G)), blk(BV_BLOCK);
    hipStream_t st = as_stream(stream);
    if (reduce)
        hipLaunchKernelGGL(bv_result_kernel<true>, grid, blk, 0, st, sums, count, N, C, G, fill, scores_out, pred);
    else
        hipLaunchKernelGGL(bv_result_kernel<false>, grid, blk, 0, st, sums, count, N, C, G, fill, scores_out, pred);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
