// Finishing a search table into the padded neighbour table the sparse layers consume, gfx950: what stood between the segmented kNN
// and the layers was a framework composition (nonzero + gather into an edge list, a distance mask, self-loop masks, cat of arange
// loops, then argsort + bincount + cumsum + scatter back into a table, with seven host reads).  One launch here.
//
// Input nbr [n_tgt, K]: global source rows; an entry outside [0, n_src) is "no neighbour" wherever it sits in its row (a search
// table pads at the end, a finished table may be fed back in).  Per row i, entries in column order:
//   keep  = in range,  and d2 <= r2 when r2 >= 0  (d = pos_tgt[i] - pos_src[j], d2 = (dx dx + dy dy) + dz dz, every operation singly
//           rounded: the form of knn.hip / collate.hip),  and j != i when self_mode is 1 or 2;
//   out [n_tgt, K_out] row i = kept entries in input order, then i itself (self_mode 2), then -1.
// counts[0] += entries written, counts[1] = max(counts[1], largest row degree): integer atomics, at most one pair per workgroup.
//
// Mapping: lanes run across columns, a group of W = next power of two >= K lanes per row, 64 / W rows per wavefront and 256 / W per
// tile of a workgroup.  The kept entries are compacted by a 64-bit ballot and a popcount of the group's lower lanes; index loads and
// stores are coalesced, the source position is a 12-byte gather made only under a radius.  The kernel streams ~8 K bytes per row.
// At most GT_MAX_BLOCKS workgroups walk over the tiles: with one workgroup per tile the two atomics per workgroup, all on the same
// two words, were the launch (194 us for 131 072 rows of K = 16, 17 MB; profiles/r20_graph_tables.md).
// graph_table_dilated_kernel (further down) is the same launch for a randomly dilated kNN graph: it draws k of a row's entries.
#include "common.hpp"

namespace crf {

constexpr int GT_BLOCK = 256;
constexpr int GT_MAX_BLOCKS = 1024;      // four workgroups for each of the 256 compute units; a workgroup walks on over the row tiles

// One (sum, max) per workgroup into counts: over the rows' first lanes inside a wavefront, then over the four wavefronts.
template <int W>
__device__ __forceinline__ void gt_publish_counts(int s, int m, unsigned long long* __restrict__ counts) {
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1);
#pragma unroll
    for (int off = WAVE / 2; off >= (W < WAVE ? W : WAVE); off >>= 1) {
        s += __shfl_xor(s, off, WAVE);
        m = max(m, __shfl_xor(m, off, WAVE));
    }
    __shared__ int w_sum[GT_BLOCK / WAVE], w_max[GT_BLOCK / WAVE];
    if (lane == 0) { w_sum[t / WAVE] = s; w_max[t / WAVE] = m; }
    __syncthreads();
    if (t == 0) {
        int bs = 0, bm = 0;
#pragma unroll
        for (int w = 0; w < GT_BLOCK / WAVE; ++w) { bs += w_sum[w]; bm = max(bm, w_max[w]); }
        if (bs > 0) atomicAdd(&counts[0], (unsigned long long)bs);
        // the maximum only grows: a workgroup that reads a value at least its own has nothing to add (a stale read only costs the
        // atomic it would have saved) -- after the first few workgroups nearly all skip it
        if ((unsigned long long)bm > __hip_atomic_load(&counts[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&counts[1], (unsigned long long)bm);
    }
}

template <int W>
__global__ __launch_bounds__(GT_BLOCK) void graph_table_kernel(const int32_t* __restrict__ nbr, int64_t n_tgt, int K, int64_t n_src,
                                                               const float* __restrict__ pos_src, const float* __restrict__ pos_tgt,
                                                               float r2, int self_mode, int32_t* __restrict__ out, int K_out,
                                                               unsigned long long* __restrict__ counts) {
    constexpr int ROWS = GT_BLOCK / W;
    const int t = (int)threadIdx.x, c = t & (W - 1), lane = t & (WAVE - 1);
    const int64_t tiles = (n_tgt + ROWS - 1) / ROWS;
    int s = 0, m = 0;                                    // entries written / largest degree of this lane's rows (kept by a row's first lane)
    // the trip count is the same for every lane of a workgroup: all of them vote in each ballot.  The next tile's entry is loaded
    // before this one is worked on, so the load's latency overlaps the stores.
    int64_t i = (int64_t)blockIdx.x * ROWS + t / W;
    int v = (i < n_tgt && c < K) ? nbr[i * K + c] : -1;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i_next = i + (int64_t)gridDim.x * ROWS;
        const int v_next = (i_next < n_tgt && c < K) ? nbr[i_next * K + c] : -1;
        const bool row_ok = i < n_tgt;
        bool keep = v >= 0 && (int64_t)v < n_src;
        if (self_mode != 0) keep = keep && (int64_t)v != i;
        if (r2 >= 0.f && keep) {
            const float* ps = pos_src + 3 * (int64_t)v;
            const float* pt = pos_tgt + 3 * i;
            const float dx = sub_rn(pt[0], ps[0]), dy = sub_rn(pt[1], ps[1]), dz = sub_rn(pt[2], ps[2]);
            const float d2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
            keep = d2 <= r2;                             // (a NaN distance is never kept)
        }
        const unsigned long long vote = __ballot(keep);
        const unsigned long long mine = W == 64 ? vote : (vote >> (lane & ~(W - 1))) & ((1ull << (W & 63)) - 1ull);
        const int kept = __popcll(mine), rank = __popcll(mine & ((1ull << c) - 1ull));
        if (row_ok) {
            int32_t* __restrict__ o = out + i * K_out;
            if (keep) o[rank] = v;
            // the rest of the row: the appended self at slot `kept`, then -1 (two trips only for the one slot past the group's width)
            for (int p = c; p < K_out; p += W)
                if (p >= kept) o[p] = (p == kept && self_mode == 2) ? (int32_t)i : -1;
            if (c == 0) {
                const int deg = kept + (self_mode == 2 ? 1 : 0);
                s += deg;
                m = max(m, deg);
            }
        }
        i = i_next;
        v = v_next;
    }
    gt_publish_counts<W>(s, m, counts);
}

// ------------------------------------------------------------------ the random dilation of a kNN graph, drawn on the search table
// The reference searches k * dilation neighbours and keeps k of them per row, drawn with replacement (models/point_conv.py:356-364,
// 385-393).  Per row i of nbr [n_tgt, K]:
//   valid  = the in-range entries in column order, have = |valid|, n_pick = min(k_pick, have);
//   pick t = valid[((h(i, t) >> 32) * have) >> 32]  for t < n_pick  (duplicates stay);
//   out [n_tgt, K_out] row i = the picks with j != i dropped under self_mode 1 / 2, in pick order, then i itself (self_mode 2), then -1.
// h is the splitmix form of sampler.hip's smp_hash under a domain of its own, keyed by (seed, *counter, salt, 64 i + t): the counter
// is ONE device word read here and never by the host, so a captured launch draws afresh once the caller has advanced it; i is the
// GLOBAL row, so a ragged batch does not equal its clouds run alone.  The multiply-shift maps the hash's upper 32 bits onto
// [0, have): every slot gets floor or ceil of 2^32 / have of them, within have / 2^32 <= 1.5e-8 of uniform.
// Mapping as above with W = next power of two >= max(K, K_out), so lane t of a row's group makes pick t.  The pick is fetched from
// the source LANE, not through LDS: the lane of the (slot + 1)-th set bit of the group's validity mask (a binary descent by popcounts),
// then one __shfl inside the group.  A second ballot compacts the kept picks like the kernel above.  Streams 4 (K + K_out) bytes per row.
constexpr unsigned long long DIL_DOMAIN = 0xA0761D6478BD642Full;

__device__ __forceinline__ unsigned long long dil_hash(unsigned long long key, unsigned long long slot) {
    unsigned long long z = key + slot * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// position of the (n + 1)-th set bit among the low W bits of m (n < their popcount)
template <int W>
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n) {
    int pos = 0;
#pragma unroll
    for (int w = W / 2; w >= 1; w >>= 1) {
        const int below = __popcll(m & ((1ull << w) - 1ull));
        if (n >= below) { n -= below; m >>= w; pos += w; }
    }
    return pos;
}

template <int W>
__global__ __launch_bounds__(GT_BLOCK) void graph_table_dilated_kernel(const int32_t* __restrict__ nbr, int64_t n_tgt, int K, int64_t n_src,
                                                                       int k_pick, unsigned long long seed,
                                                                       const long long* __restrict__ counter, unsigned long long salt,
                                                                       int self_mode, int32_t* __restrict__ out, int K_out,
                                                                       unsigned long long* __restrict__ counts) {
    constexpr int ROWS = GT_BLOCK / W;
    const int t = (int)threadIdx.x, c = t & (W - 1), lane = t & (WAVE - 1);
    const int64_t tiles = (n_tgt + ROWS - 1) / ROWS;
    const unsigned long long key = (seed ^ DIL_DOMAIN) + 0x9E3779B97F4A7C15ull * ((unsigned long long)*counter + 1ull)
                                   + salt * 0xC2B2AE3D27D4EB4Full;
    int s = 0, m = 0;
    // every lane of a workgroup makes the same trips (ballots and shuffles need them all); the next tile's entry is loaded first
    int64_t i = (int64_t)blockIdx.x * ROWS + t / W;
    int v = (i < n_tgt && c < K) ? nbr[i * K + c] : -1;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i_next = i + (int64_t)gridDim.x * ROWS;
        const int v_next = (i_next < n_tgt && c < K) ? nbr[i_next * K + c] : -1;
        const bool row_ok = i < n_tgt;
        const bool valid = v >= 0 && (int64_t)v < n_src;
        const unsigned long long have_vote = __ballot(valid);
        const unsigned long long mask = W == 64 ? have_vote : (have_vote >> (lane & ~(W - 1))) & ((1ull << (W & 63)) - 1ull);
        const int have = __popcll(mask);
        const bool picks = c < min(k_pick, have);        // this lane makes pick t = c
        int from = c;
        if (picks) {
            const unsigned long long h = dil_hash(key, (unsigned long long)i * 64ull + (unsigned long long)c);
            from = nth_set_bit<W>(mask, (int)(((h >> 32) * (unsigned long long)have) >> 32));
        }
        const int j = __shfl(v, from, W);                // (all lanes take part; `from` is a lane of this row's own group)
        const bool keep = picks && (self_mode == 0 || (int64_t)j != i);
        const unsigned long long vote = __ballot(keep);
        const unsigned long long mine = W == 64 ? vote : (vote >> (lane & ~(W - 1))) & ((1ull << (W & 63)) - 1ull);
        const int kept = __popcll(mine), rank = __popcll(mine & ((1ull << c) - 1ull));
        if (row_ok) {
            int32_t* __restrict__ o = out + i * K_out;
            if (keep) o[rank] = j;
            if (c >= kept && c < K_out) o[c] = (c == kept && self_mode == 2) ? (int32_t)i : -1;      // (W >= K_out: one slot per lane)
            if (c == 0) {
                const int deg = kept + (self_mode == 2 ? 1 : 0);
                s += deg;
                m = max(m, deg);
            }
        }
        i = i_next;
        v = v_next;
    }
    gt_publish_counts<W>(s, m, counts);
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_graph_table(const int32_t* nbr, int64_t n_tgt, int K, int64_t n_src, const float* pos_src,
                                   const float* pos_tgt, float r2, int self_mode, int32_t* out, int K_out, int64_t* counts,
                                   crf_stream_t stream) {
    CRF_REQUIRE(nbr && out && counts && (const void*)out != (const void*)nbr, CRF_ERR_ARG, "null pointer or aliasing");
    CRF_REQUIRE(K >= 1 && K <= 64, CRF_ERR_ARG, "K=%d outside [1, 64]", K);
    CRF_REQUIRE(self_mode >= 0 && self_mode <= 2, CRF_ERR_ARG, "self_mode=%d outside {0, 1, 2}", self_mode);
    CRF_REQUIRE(K_out == K + (self_mode == 2 ? 1 : 0), CRF_ERR_ARG, "K_out=%d, expected %d (K=%d, self_mode=%d)", K_out,
                K + (self_mode == 2 ? 1 : 0), K, self_mode);
    CRF_REQUIRE(n_tgt >= 0 && n_src >= 0, CRF_ERR_ARG, "negative size (n_tgt=%lld n_src=%lld)", (long long)n_tgt, (long long)n_src);
    CRF_REQUIRE(self_mode == 0 || n_src == n_tgt, CRF_ERR_ARG, "self_mode=%d needs n_src == n_tgt (got %lld, %lld)", self_mode,
                (long long)n_src, (long long)n_tgt);
    CRF_REQUIRE(!(r2 >= 0.f) || (pos_src && pos_tgt), CRF_ERR_ARG, "a radius cut needs both position arrays");
    CRF_REQUIRE(n_tgt * K_out < (int64_t)1 << 31, CRF_ERR_ARG, "edge ids exceed int32 (n_tgt=%lld K_out=%d)", (long long)n_tgt, K_out);
    if (n_tgt == 0) return CRF_OK;
    int W = 1;
    while (W < K) W <<= 1;
    const int64_t tiles = cdiv(n_tgt, GT_BLOCK / W);
    const dim3 grid((unsigned)(tiles < GT_MAX_BLOCKS ? tiles : GT_MAX_BLOCKS)), blk(GT_BLOCK);
    hipStream_t st = as_stream(stream);
    if (!(r2 >= 0.f)) r2 = -1.f;                         // (NaN: no cut, like every negative value)
    const bool known = dispatch_width(Widths<1, 2, 4, 8, 16, 32, 64>{}, W, [&](auto Wc) {
        hipLaunchKernelGGL(graph_table_kernel<decltype(Wc)::value>, grid, blk, 0, st, nbr, n_tgt, K, n_src, pos_src, pos_tgt, r2,
                           self_mode, out, K_out, reinterpret_cast<unsigned long long*>(counts));
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "no lane-group width for K=%d", K);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_graph_table_dilated(const int32_t* nbr, int64_t n_tgt, int K, int64_t n_src, int k_pick, uint64_t seed,
                                           const int64_t* counter, int64_t salt, int self_mode, int32_t* out, int K_out,
                                           int64_t* counts, crf_stream_t stream) {
    CRF_REQUIRE(nbr && out && counts && counter && (const void*)out != (const void*)nbr, CRF_ERR_ARG, "null pointer or aliasing");
    CRF_REQUIRE(K >= 1 && K <= 64, CRF_ERR_ARG, "K=%d outside [1, 64]", K);
    CRF_REQUIRE(k_pick >= 1 && k_pick <= 64, CRF_ERR_ARG, "k_pick=%d outside [1, 64]", k_pick);
    CRF_REQUIRE(self_mode >= 0 && self_mode <= 2, CRF_ERR_ARG, "self_mode=%d outside {0, 1, 2}", self_mode);
    CRF_REQUIRE(K_out == k_pick + (self_mode == 2 ? 1 : 0) && K_out <= 64, CRF_ERR_ARG,
                "K_out=%d, expected %d and at most 64 (k_pick=%d, self_mode=%d)", K_out, k_pick + (self_mode == 2 ? 1 : 0), k_pick, self_mode);
    CRF_REQUIRE(n_tgt >= 0 && n_src >= 0, CRF_ERR_ARG, "negative size (n_tgt=%lld n_src=%lld)", (long long)n_tgt, (long long)n_src);
    CRF_REQUIRE(self_mode == 0 || n_src == n_tgt, CRF_ERR_ARG, "self_mode=%d needs n_src == n_tgt (got %lld, %lld)", self_mode,
                (long long)n_src, (long long)n_tgt);
    CRF_REQUIRE(n_tgt * K_out < (int64_t)1 << 31, CRF_ERR_ARG, "edge ids exceed int32 (n_tgt=%lld K_out=%d)", (long long)n_tgt, K_out);
    CRF_REQUIRE(salt >= 0, CRF_ERR_ARG, "salt=%lld is negative", (long long)salt);
    if (n_tgt == 0) return CRF_OK;
    int W = 1;
    while (W < K || W < K_out) W <<= 1;
    const int64_t tiles = cdiv(n_tgt, GT_BLOCK / W);
    const dim3 grid((unsigned)(tiles < GT_MAX_BLOCKS ? tiles : GT_MAX_BLOCKS)), blk(GT_BLOCK);
    hipStream_t st = as_stream(stream);
    const bool known = dispatch_width(Widths<1, 2, 4, 8, 16, 32, 64>{}, W, [&](auto Wc) {
        hipLaunchKernelGGL(graph_table_dilated_kernel<decltype(Wc)::value>, grid, blk, 0, st, nbr, n_tgt, K, n_src, k_pick,
                           (unsigned long long)seed, reinterpret_cast<const long long*>(counter), (unsigned long long)salt, self_mode,
                           out, K_out, reinterpret_cast<unsigned long long*>(counts));
    });
    CRF_REQUIRE(known, CRF_ERR_UNSUPPORTED, "no lane-group width for K=%d, K_out=%d", K, K_out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
