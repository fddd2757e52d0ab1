// The possibility sampler of datasets/semantic3d_dataset.py:423-460 (`_get_random`): seed = arg-min possibility, crop = the
// num_points nearest points of the (jittered) seed, possibility += (1 - d / d_max)^2 * weight.  Three forms, one arithmetic
// (crop_common.hpp: the key, the distances, the gain, the row write, the arg-min):
//   single cloud   crfconv_argmin_f64 + crfconv_possibility_crop: the caller picks the seed, the entry sorts the keys of EVERY point
//                  (a full stable radix sort) and takes the first k.  The independent twin the batch forms are tested against.
//   batch          crfconv_possibility_crop_batch: B crops per call, decided and written on the device (B consecutive __getitem__
//                  calls; crfconv_amd.sampling.PossibilitySampler.get_batch).  No host read anywhere, no scratch memory: the whole
//                  call can sit in a captured hipGraph (data.CollateGraph(sampler=)).  Bit for bit what B calls of the single form
//                  give for the same jitter and shuffle, without sorting the cloud.
//   S3DIS batch    crfconv_possibility_crop_batch_s3dis: the same for rooms that may be smaller than a crop (below).
//
//   ONE sequence per crop b for both batch forms (sb_run), in stream order (crop b + 1 sees the possibilities crop b left):
//     sb_choose_kernel   1 workgroup: cloud = arg-min of the per-cloud minima (first index on ties), seed point = that cloud's
//                        arg-min, jitter (Box-Muller in float64 on 53-bit uniforms of smp_hash, or noise_in), centre; clears the
//                        select's histograms.  The cloud is read through a DEVICE table of descriptors (crf_cloud_desc), the grids
//                        below are sized for the largest cloud and leave early beyond the chosen one.
//     sb_hist_kernel x 8 MSB-first radix SELECT on the 64-bit key (crop_key: bit pattern of the float64 squared distance, recomputed
//                        from the 12-byte point in every pass): pass p counts digit p of the keys that match the p digits found so far
//                        (per-wavefront LDS bins; a wavefront whose matching lanes agree on the digit -- the rule in the exponent
//                        passes -- adds one popcount; <= 256 global integer atomics per workgroup).  Every workgroup resolves the
//                        PREVIOUS pass itself (256-bin scan: the digit holding rank `want`, and the rank inside it), so there is
//                        no one-workgroup launch between the passes.  Reads 12 B per point and pass, writes nothing of size n.
//     sb_count_kernel    resolves the last digit (the k-th key is now known) and counts per tile of 4096 points the keys below it
//                        and equal to it.
//     sb_scatter_kernel  ORDER-PRESERVING compaction (ballot ranks inside a wavefront, tile bases summed from the counts): keys
//                        below the k-th in point order into [0, L), then the first k - L points with the k-th key in point order.
//     rsort_pairs_u64    the library's stable radix sort over those k pairs only: (key, point id) order, i.e. what the full stable
//                        sort of the single form yields; ties at the ball's boundary go to the lower point id.
//     (S3DIS form only)  the padding of a short crop, see below: sb_perm_compact_kernel, sb_choice_keys_kernel + its sort,
//                        sb_choice_final_kernel -- each enqueued only when the table or the caller's outputs can need it.
//     sb_dist_kernel / sb_update_kernel   float32 distances, d_max, possibility += (1 - d / d_max)^2 weight, and row b of the batch:
//                        pos, x = [pos, rgb], y, point_idx, through the shuffle.
//     sb_argmin_partial_kernel / sb_argmin_final_kernel   the chosen cloud's new minimum possibility (:451).
//   once per call: the B shuffles.  perm_b = stable arg-sort over t of smp_hash(seed, counter, b, 8 + t): ONE sort of the B k hashes
//   (values b k + t) followed by one stable pass on b -- the crops do not enter, so this is not repeated per crop.
//   Launches, where a pass of the radix sort is 4 (histogram, two for the scan, scatter: k = 40 960 .. 65 536): 47 per crop --
//   1 choose + 8 + 1 count + 1 scatter + 8 x 4 + distance + update + 2 arg-min -- + 39 per call for the device's own shuffles
//   (keys, 8 x 4, crop keys, 1 x 4 for B <= 256, final); the S3DIS form adds per crop only what its table can need.
//
//   Where the forms differ (template argument S3DIS of the choose, scatter, distance and update kernels;
//   datasets/s3dis_dataset.py:343-379, crfconv_possibility_crop_batch_s3dis): the S3DIS form selects kc = min(n, k) rows -- a device
//   value; rows kc .. k of the sort's input are all-ones sentinels --, centres all three axes, takes the distances of the float32
//   centred coordinates, has no point weight, and pads a crop of kc < k rows to k rows through `choice`.
// Everything is integer counting or singly rounded arithmetic in a fixed order: deterministic, no floating-point atomics.
#include <cmath>

#include "crop_common.hpp"
#include "radix_sort.hpp"

namespace crf {

constexpr int SB_NT = CROP_NT, SB_IPT = 16, SB_TILE = SB_NT * SB_IPT;  // threads per workgroup; points per thread / per tile
constexpr int SB_ARGMIN_BLOCKS = 1024;                                // workgroups of an arg-min's first pass, every form
constexpr unsigned long long SMP_DOMAIN = 0x8CB92BA72F3D8DD7ull;       // separates these draws from the subsets' / dropout's / augmentation's
constexpr int SMP_PERM_SLOT = 8;                                       // slots 0 .. 5: the jitter's uniforms; 8 + t: shuffle key of row t

// host twin: sampling._smp_hash
__device__ __forceinline__ unsigned long long smp_hash(unsigned long long seed, unsigned long long ctr, unsigned long long b,
                                                       unsigned long long slot) {
    unsigned long long z = (seed ^ SMP_DOMAIN) + 0x9E3779B97F4A7C15ull * (ctr + 1ull) + b * 0xC2B2AE3D27D4EB4Full
                           + slot * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double smp_u53(unsigned long long h) { return (double)((h >> 11) + 1ull) * 0x1p-53; }      // (0, 1]

struct SbSel {                    // the select after p passes: the digits found (high-aligned) and the rank wanted among the keys that match
    unsigned long long prefix;
    long long want;
};
struct SbCrop {                   // one crop's device-side decisions; lives in the workspace, rewritten per crop
    SbSel sel[9];
    double center[3];
    long long n;
    int cloud, pad;
    long long kc;                 // rows of this crop: k, or min(n, k) in the S3DIS form (a small room is taken whole)
};

template <bool S3DIS>
__global__ __launch_bounds__(SB_NT) void sb_choose_kernel(const crf_cloud_desc* __restrict__ clouds, int n_clouds,
                                                          const double* __restrict__ minv, const int64_t* __restrict__ mini,
                                                          unsigned long long seed, const int64_t* __restrict__ counter, int b, long long k,
                                                          double noise_scale, const double* __restrict__ noise_in, SbCrop* __restrict__ st,
                                                          int32_t* __restrict__ hist, double* __restrict__ noise_out,
                                                          double* __restrict__ out_center, int64_t* __restrict__ out_cloud) {
#pragma unroll
    for (int p = 0; p < 8; ++p) hist[p * 256 + threadIdx.x] = 0;
    if (threadIdx.x >= WAVE) return;
    const int lane = threadIdx.x;
    MinIdx m = min_none();
    for (int c = lane; c < n_clouds; c += WAVE) m = min_first(m, MinIdx{minv[c], (long long)c});
    m = wave_min_first(m);
    const int c = m.i < (long long)n_clouds ? (int)m.i : 0;          // (all minima NaN: cloud 0)
    const crf_cloud_desc cd = clouds[c];
    long long pick = mini[c];
    if (pick < 0 || pick >= cd.n) pick = 0;
    if (lane < 3) {
        double nz;
        if (noise_in != nullptr) {
            nz = noise_in[3 * b + lane];
        } else {
            const unsigned long long ctr = (unsigned long long)*counter;
            const double u1 = smp_u53(smp_hash(seed, ctr, (unsigned long long)b, 2ull * lane));
            const double u2 = smp_u53(smp_hash(seed, ctr, (unsigned long long)b, 2ull * lane + 1ull));
            nz = dmul_rn(sqrt(-2.0 * log(u1)) * cospi(2.0 * u2), noise_scale);
        }
        const double ce = (double)cd.points[3 * pick + lane] + nz;      // :426-430
        st->center[lane] = ce;
        if (out_center != nullptr) out_center[3 * b + lane] = ce;
        if (noise_out != nullptr) noise_out[3 * b + lane] = nz;
    }
    if (lane == 0) {
        st->cloud = c;
        st->n = cd.n;
        const long long kc = S3DIS && cd.n < k ? cd.n : k;            // s3dis_dataset.py:352-355
        st->kc = kc;
        st->sel[0] = SbSel{0ull, kc};
        if (out_cloud != nullptr) out_cloud[b] = c;
    }
}

// The select after pass `prev`, from its histogram: the smallest digit whose inclusive count reaches `want`.  Whole workgroup.
__device__ __forceinline__ SbSel sb_resolve(const SbCrop* __restrict__ st, const int32_t* __restrict__ hist, int prev) {
    __shared__ long long s_w[SB_NT / WAVE];
    __shared__ long long s_pick[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const SbSel s = st->sel[prev];
    const long long h = hist[prev * 256 + t];
    long long inc = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(inc, o, WAVE); if (lane >= o) inc += u; }
    if (lane == 63) s_w[wave] = inc;
    if (t == 0) { s_pick[0] = 255; s_pick[1] = 0; }                    // (fewer than `want` keys: cannot happen for k <= n)
    __syncthreads();
    for (int w = 0; w < wave; ++w) inc += s_w[w];
    if (inc - h < s.want && s.want <= inc) { s_pick[0] = t; s_pick[1] = inc - h; }
    __syncthreads();
    SbSel r;
    r.prefix = s.prefix | ((unsigned long long)s_pick[0] << (56 - 8 * prev));
    r.want = s.want - s_pick[1];
    __syncthreads();                                                 // (the shared words are reused by the caller's next resolve)
    return r;
}

__global__ __launch_bounds__(SB_NT) void sb_hist_kernel(const crf_cloud_desc* __restrict__ clouds, SbCrop* __restrict__ st,
                                                        int32_t* __restrict__ hist, int p) {
    __shared__ int s_h[SB_NT / WAVE][256];
    const long long n = st->n, lo = (long long)blockIdx.x * SB_TILE;
    if (lo >= n) return;                                               // uniform: the grid is sized for the largest cloud
    SbSel s = st->sel[0];
    if (p > 0) {
        s = sb_resolve(st, hist, p - 1);
        if (blockIdx.x == 0 && threadIdx.x == 0) st->sel[p] = s;       // (every workgroup finds the same; the next launch reads it)
    }
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int w = 0; w < SB_NT / WAVE; ++w) s_h[w][t] = 0;
    __syncthreads();
    const float* __restrict__ pts = clouds[st->cloud].points;
    const double cx = st->center[0], cy = st->center[1], cz = st->center[2];
    const int shift = 56 - 8 * p;
    const unsigned long long want_hi = p > 0 ? (s.prefix >> (shift + 8)) : 0ull;
    int* h = s_h[wave];
    for (int r = 0; r < SB_IPT; ++r) {
        const long long i = lo + (long long)r * SB_NT + t;
        bool match = i < n;
        unsigned d = 0;
        if (match) {
            const unsigned long long key = crop_key(pts, i, cx, cy, cz);
            if (p > 0) match = (key >> (shift + 8)) == want_hi;
            d = (unsigned)((key >> shift) & 255ull);
        }
        const unsigned long long act = __ballot(match);
        if (act == 0ull) continue;                                     // uniform per wavefront
        const int first = __ffsll((long long)act) - 1;
        const unsigned d0 = (unsigned)__shfl((int)d, first, WAVE);
        if (__ballot(match && d == d0) == act) {                       // one digit in the wavefront: one add (the exponent passes)
            if (lane == first) atomicAdd(&h[d0], __popcll(act));
        } else if (match) {
            atomicAdd(&h[d], 1);
        }
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < SB_NT / WAVE; ++w) total += s_h[w][t];
    if (total != 0) atomicAdd(&hist[p * 256 + t], total);
}

__global__ __launch_bounds__(SB_NT) void sb_count_kernel(const crf_cloud_desc* __restrict__ clouds, SbCrop* __restrict__ st,
                                                         const int32_t* __restrict__ hist, int32_t* __restrict__ cnt, long long nb) {
    __shared__ int s_c[SB_NT / WAVE][2];
    const long long n = st->n, lo = (long long)blockIdx.x * SB_TILE;
    if (lo >= n) return;
    const SbSel s = sb_resolve(st, hist, 7);                           // prefix = the k-th key, want = how many points with that key are taken
    if (blockIdx.x == 0 && threadIdx.x == 0) st->sel[8] = s;
    const int t = threadIdx.x;
    const float* __restrict__ pts = clouds[st->cloud].points;
    const double cx = st->center[0], cy = st->center[1], cz = st->center[2];
    int less = 0, eq = 0;
    for (int r = 0; r < SB_IPT; ++r) {
        const long long i = lo + (long long)r * SB_NT + t;
        if (i < n) {
            const unsigned long long key = crop_key(pts, i, cx, cy, cz);
            less += key < s.prefix ? 1 : 0;
            eq += key == s.prefix ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { less += __shfl_xor(less, o, WAVE); eq += __shfl_xor(eq, o, WAVE); }
    if ((t & 63) == 0) { s_c[t >> 6][0] = less; s_c[t >> 6][1] = eq; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < SB_NT / WAVE; ++w) { less += s_c[w][0]; eq += s_c[w][1]; }
        cnt[blockIdx.x] = less;
        cnt[nb + blockIdx.x] = eq;
    }
}

template <bool S3DIS>
__global__ __launch_bounds__(SB_NT) void sb_scatter_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                           const int32_t* __restrict__ cnt, long long nb, long long k,
                                                           unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ long long s_b[SB_NT / WAVE][2];
    __shared__ int s_l[SB_NT / WAVE], s_e[SB_NT / WAVE];
    const long long n = st->n, lo = (long long)blockIdx.x * SB_TILE;
    if constexpr (S3DIS) {                                             // rows kc .. k of the sort's input: sentinels that sort last
        const long long kc = st->kc;
        for (long long i = kc + (long long)blockIdx.x * SB_NT + threadIdx.x; i < k; i += (long long)gridDim.x * SB_NT) {
            keys_out[i] = ~0ull;
            vals_out[i] = 0xFFFFFFFFu;
        }
        k = kc;
    }
    if (lo >= n) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long kth = st->sel[8].prefix;
    const long long want = st->sel[8].want, L = k - want;
    // first slots of this tile: the counts of the tiles before it (integer sums, any order)
    long long bl = 0, be = 0;
    for (long long i = t; i < (long long)blockIdx.x; i += SB_NT) { bl += cnt[i]; be += cnt[nb + i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { bl += __shfl_xor(bl, o, WAVE); be += __shfl_xor(be, o, WAVE); }
    if (lane == 0) { s_b[wave][0] = bl; s_b[wave][1] = be; }
    __syncthreads();
    bl = 0; be = 0;
#pragma unroll
    for (int w = 0; w < SB_NT / WAVE; ++w) { bl += s_b[w][0]; be += s_b[w][1]; }
    if (bl >= L && be >= want) return;                                  // uniform: nothing of this tile is taken
    const float* __restrict__ pts = clouds[st->cloud].points;
    const double cx = st->center[0], cy = st->center[1], cz = st->center[2];
    for (int r = 0; r < SB_IPT; ++r) {
        const long long i = lo + (long long)r * SB_NT + t;
        unsigned long long key = ~0ull;
        if (i < n) key = crop_key(pts, i, cx, cy, cz);
        const bool less = i < n && key < kth, eq = i < n && key == kth;
        const unsigned long long ml = compact_count(less, s_l), me = compact_count(eq, s_e);
        __syncthreads();
        int tl, te;
        const long long sl = compact_slot(ml, s_l, bl, tl), se = compact_slot(me, s_e, be, te);
        if (less) {
            if (sl < L) { keys_out[sl] = key; vals_out[sl] = (uint32_t)i; }
        } else if (eq) {
            if (se < want) { keys_out[L + se] = key; vals_out[L + se] = (uint32_t)i; }
        }
        bl += tl;
        be += te;
        __syncthreads();
    }
}

// dist[t] = the update's float32 distance of selected row t (crop_row_dist) and the workgroup maxima; S3DIS: rows kc .. k hold 0
template <bool S3DIS>
__global__ __launch_bounds__(SB_NT) void sb_dist_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                        const uint32_t* __restrict__ sel, long long k, float* __restrict__ dist,
                                                        float* __restrict__ pmax) {
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    const float* __restrict__ points = clouds[st->cloud].points;
    float d = 0.f;
    if (t < k) {
        const long long i = sel[t];
        if ((!S3DIS || t < st->kc) && i < st->n) d = crop_row_dist<S3DIS>(points, i, st->center);
        dist[t] = d;
    }
    block_max_to(d, pmax);
}

// possibility += (1 - d / d_max)^2 [weight] over the crop's DISTINCT rows and row t of the batch through the shuffle.
//   Semantic3D: row t shows selected element perm[t], and that element's possibility is updated by the same thread.
//   S3DIS (s3dis_dataset.py:364-365, :357, :375-377): thread t < kc updates selected element t, weight 1; row t of the batch = row
//   choice[t] of the shuffled crop = selected element perm[choice[t]], perm the device's own shuffle restricted to kc rows
//   (perm_compact) when the crop is short.  kc == k: choice is the identity and is not read.
template <bool S3DIS>
__global__ __launch_bounds__(SB_NT) void sb_update_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                          const uint32_t* __restrict__ sel, const int64_t* __restrict__ perm,
                                                          const int64_t* __restrict__ perm_compact, const int64_t* __restrict__ choice,
                                                          long long k, const float* __restrict__ dist, const float* __restrict__ pmax,
                                                          int nblk, float* __restrict__ out_pos, float* __restrict__ out_x, int xc,
                                                          int64_t* __restrict__ out_y, int64_t* __restrict__ out_idx) {
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (t >= k) return;
    const crf_cloud_desc cd = clouds[st->cloud];
    long long kc = k, s = t;
    if constexpr (S3DIS) {
        kc = st->kc;
        if (t < kc) {
            const long long j = sel[t];
            if (j < cd.n) cd.possibility[j] += (double)crop_gain(dist[t], crop_dmax(pmax, nblk));
        }
        if (kc < k) {
            if (choice == nullptr) return;
            s = choice[t];
            if (perm_compact != nullptr) perm = perm_compact;
        }
        if (s < 0 || s >= kc) return;
    }
    const long long src = perm ? perm[s] : s;
    if (src < 0 || src >= kc) return;
    const long long i = sel[src];
    if (i >= cd.n) return;
    if constexpr (!S3DIS) {
        const float sq = crop_gain(dist[src], crop_dmax(pmax, nblk));
        cd.possibility[i] += cd.point_weight ? dmul_rn((double)sq, cd.point_weight[i]) : (double)sq;
    }
    crop_write_row<S3DIS>(cd.points, cd.rgb, cd.labels, i, st->center, t, out_pos, out_x, xc, out_y, out_idx);
}

__global__ __launch_bounds__(SB_NT) void sb_argmin_partial_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                                  double* __restrict__ pv, int64_t* __restrict__ pi) {
    const double* __restrict__ v = clouds[st->cloud].possibility;
    const long long n = st->n;
    MinIdx m = min_none();
    for (long long i = (long long)blockIdx.x * SB_NT + threadIdx.x; i < n; i += (long long)gridDim.x * SB_NT)
        m = min_first(m, MinIdx{v[i], i});
    m = block_min_first(m);
    if (threadIdx.x == 0) { pv[blockIdx.x] = m.v; pi[blockIdx.x] = m.i; }
}
__global__ __launch_bounds__(SB_NT) void sb_argmin_final_kernel(const SbCrop* __restrict__ st, const double* __restrict__ pv,
                                                                const int64_t* __restrict__ pi, int nblk, double* __restrict__ minv,
                                                                int64_t* __restrict__ mini) {
    MinIdx m = min_none();
    for (int b = threadIdx.x; b < nblk; b += SB_NT) m = min_first(m, MinIdx{pv[b], (long long)pi[b]});
    m = block_min_first(m);
    if (threadIdx.x == 0) { minv[st->cloud] = m.v; mini[st->cloud] = m.i; }
}

// ---- the shuffles
__global__ __launch_bounds__(SB_NT) void sb_perm_keys_kernel(unsigned long long seed, const int64_t* __restrict__ counter, long long k,
                                                             long long total, unsigned long long* __restrict__ keys,
                                                             uint32_t* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (i >= total) return;
    const unsigned long long b = (unsigned long long)(i / k), t = (unsigned long long)(i % k);
    keys[i] = smp_hash(seed, (unsigned long long)*counter, b, (unsigned long long)SMP_PERM_SLOT + t);
    vals[i] = (uint32_t)i;
}
__global__ __launch_bounds__(SB_NT) void sb_perm_crop_keys_kernel(const uint32_t* __restrict__ vals, long long k, long long total,
                                                                  unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (i < total) keys[i] = (unsigned long long)(vals[i] / (unsigned long long)k);
}
__global__ __launch_bounds__(SB_NT) void sb_perm_final_kernel(const uint32_t* __restrict__ vals, long long k, long long total,
                                                              int64_t* __restrict__ perm, int64_t* __restrict__ perm_out) {
    const long long i = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (i >= total) return;
    const int64_t v = (int64_t)(vals[i] % (unsigned long long)k);
    perm[i] = v;
    if (perm_out != nullptr) perm_out[i] = v;
}

// ---- the padding of the S3DIS form: a room smaller than k is taken whole (kc = n rows) and padded to k rows by `choice`.
constexpr unsigned long long SMP_CHOICE_SLOT = 1ull << 32;             // slot (j + 1) 2^32 + t: padding key of element t of block j

// The shuffle of a crop of kc < k rows: the stable ranking of the first kc hashes of row b = the entries below kc of the row's full
// arg-sort, in their order.  One workgroup, order-preserving compaction; perm_out (or NULL) <- the kc entries, then -1.
__global__ __launch_bounds__(SB_NT) void sb_perm_compact_kernel(const SbCrop* __restrict__ st, const int64_t* __restrict__ full, long long k,
                                                                int64_t* __restrict__ compact, int64_t* __restrict__ perm_out) {
    __shared__ int s_c[SB_NT / WAVE];
    const long long kc = st->kc;
    const int t = threadIdx.x;
    if (kc >= k) {
        if (perm_out != nullptr)
            for (long long i = t; i < k; i += SB_NT) perm_out[i] = full[i];
        return;
    }
    long long base = 0;
    for (long long lo = 0; lo < k; lo += SB_NT) {
        const long long i = lo + t;
        const long long v = i < k ? full[i] : k;
        const bool keep = v < kc;
        const unsigned long long m = compact_count(keep, s_c);
        __syncthreads();
        int total;
        const long long slot = compact_slot(m, s_c, base, total);
        if (keep) {
            compact[slot] = v;
            if (perm_out != nullptr) perm_out[slot] = v;
        }
        base += total;
        __syncthreads();
    }
    if (perm_out != nullptr)
        for (long long i = kc + t; i < k; i += SB_NT) perm_out[i] = -1;
}

// Padding of a crop of kc < k rows (FixedPoints(k, replace=False, allow_duplicates=True), :375-377): ceil(k / kc) independent
// permutations of range(kc) laid end to end, the first k entries.  Permutation j = stable arg-sort over t of the upper 32 bits of
// smp_hash(seed, counter, b, (j + 1) 2^32 + t): ONE sort of at most k + kc - 1 < 2 k pairs keyed (j, hash); grid of 2 k elements.
__global__ __launch_bounds__(SB_NT) void sb_choice_keys_kernel(const SbCrop* __restrict__ st, unsigned long long seed,
                                                               const int64_t* __restrict__ counter, int b, long long k,
                                                               unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long e = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (e >= 2 * k) return;
    const long long kc = st->kc;
    unsigned long long key = ~0ull;
    if (kc < k && kc > 0) {
        const long long nblocks = (k + kc - 1) / kc;
        if (e < nblocks * kc) {
            const unsigned long long j = (unsigned long long)(e / kc), t = (unsigned long long)(e % kc);
            key = (j << 32) | (smp_hash(seed, (unsigned long long)*counter, (unsigned long long)b, (j + 1ull) * SMP_CHOICE_SLOT + t) >> 32);
        }
    }
    keys[e] = key;
    vals[e] = (uint32_t)e;
}
__global__ __launch_bounds__(SB_NT) void sb_choice_final_kernel(const SbCrop* __restrict__ st, const uint32_t* __restrict__ vals, long long k,
                                                                int64_t* __restrict__ choice, int64_t* __restrict__ choice_out) {
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (t >= k) return;
    const long long kc = st->kc;
    const int64_t v = kc < k && kc > 0 && vals != nullptr ? (int64_t)vals[t] - (t / kc) * kc : t;      // sorted slot t lies in block t / kc
    choice[t] = v;
    if (choice_out != nullptr) choice_out[t] = v;
}

// ------------------------------------------------------------------------------------------ the single-cloud form
// arg-min with the first index on ties (np.argmin; crop_common.hpp), two passes: per-block candidates, then one block.
__global__ __launch_bounds__(SB_NT) void argmin_partial_kernel(const double* __restrict__ v, int64_t n,
                                                               double* __restrict__ pv, int64_t* __restrict__ pi) {
    MinIdx m = min_none();
    for (int64_t i = (int64_t)blockIdx.x * SB_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * SB_NT)
        m = min_first(m, MinIdx{v[i], i});
    m = block_min_first(m);
    if (threadIdx.x == 0) { pv[blockIdx.x] = m.v; pi[blockIdx.x] = m.i; }
}

__global__ __launch_bounds__(SB_NT) void argmin_final_kernel(const double* __restrict__ pv,
                                                             const int64_t* __restrict__ pi, int nblk,
                                                             double* __restrict__ out_v, int64_t* __restrict__ out_i) {
    MinIdx m = min_none();
    for (int b = threadIdx.x; b < nblk; b += SB_NT) m = min_first(m, MinIdx{pv[b], pi[b]});
    m = block_min_first(m);
    if (threadIdx.x == 0) { *out_v = m.v; *out_i = m.i; }
}

// pick point = float64(points[pick]) + noise (semantic3d_dataset.py:426-430)
__global__ void pick_point_kernel(const float* __restrict__ points, const int64_t* __restrict__ pick,
                                  const double* __restrict__ noise, double* __restrict__ center) {
    if (threadIdx.x < 3) center[threadIdx.x] = (double)points[*pick * 3 + threadIdx.x] + (noise ? noise[threadIdx.x] : 0.0);
}

// The key of EVERY point for a full stable sort of the cloud -- the independent twin of the batch forms' select -- then the
// distances, the update and the row write of crop_common.hpp in the Semantic3D form.
__global__ __launch_bounds__(SB_NT) void crop_keys_kernel(const float* __restrict__ points, int64_t n,
                                                          const double* __restrict__ center,
                                                          unsigned long long* __restrict__ keys,
                                                          unsigned int* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * SB_NT + threadIdx.x;
    if (i >= n) return;
    keys[i] = crop_key(points, i, center[0], center[1], center[2]);
    ids[i] = (unsigned int)i;
}

__global__ __launch_bounds__(SB_NT) void crop_dist_kernel(const float* __restrict__ points,
                                                          const unsigned int* __restrict__ sel, int64_t k,
                                                          const double* __restrict__ center,
                                                          float* __restrict__ dist, float* __restrict__ pmax) {
    const int64_t t = (int64_t)blockIdx.x * SB_NT + threadIdx.x;
    float d = 0.f;
    if (t < k) dist[t] = d = crop_row_dist<false>(points, sel[t], center);
    block_max_to(d, pmax);
}

// possibility[q] += (1 - d / d_max)^2 * weight[label_to_idx(labels[q])]     (:449-450), and the crop's outputs
__global__ __launch_bounds__(SB_NT) void crop_update_kernel(const float* __restrict__ points,
                                                            const unsigned int* __restrict__ sel,
                                                            const int64_t* __restrict__ perm, int64_t k,
                                                            const double* __restrict__ center,
                                                            const float* __restrict__ dist,
                                                            const float* __restrict__ pmax, int nblk,
                                                            const double* __restrict__ point_weight,
                                                            double* __restrict__ possibility,
                                                            int64_t* __restrict__ out_idx,
                                                            float* __restrict__ out_xyz) {
    const int64_t t = (int64_t)blockIdx.x * SB_NT + threadIdx.x;
    if (t >= k) return;
    const int64_t src = perm ? perm[t] : t;            // output row t shows selected element perm[t] (the shuffle)
    const int64_t i = sel[src];
    const float sq = crop_gain(dist[src], crop_dmax(pmax, nblk));
    // the weights are float64 for train / val (class_weight array) and the python int 1 for test (float32 result)
    possibility[i] += point_weight ? dmul_rn((double)sq, point_weight[i]) : (double)sq;      // rows of a crop are distinct points
    crop_write_row<false>(points, nullptr, nullptr, i, center, t, out_xyz, nullptr, 0, nullptr, out_idx);
}

struct CropWs {                   // workspace of the single-crop entry
    unsigned long long *keys_in, *keys_out;
    unsigned int *ids_in, *ids_out;
    float *dist, *pmax;
    double* center;
    char* sort;
    size_t bytes;
};
static CropWs crop_carve(void* workspace, int64_t n, int64_t k) {
    Carve c(workspace);
    CropWs w;
    w.keys_in = c.take<unsigned long long>((size_t)n);
    w.keys_out = c.take<unsigned long long>((size_t)n);
    w.ids_in = c.take<unsigned int>((size_t)n);
    w.ids_out = c.take<unsigned int>((size_t)n);
    w.dist = c.take<float>((size_t)k);
    w.pmax = c.take<float>((size_t)cdiv(k, SB_NT));
    w.center = c.take<double>(3);
    w.sort = c.take<char>(rsort_workspace(n));      // this library's radix sort (radix_sort.hpp)
    w.bytes = c.bytes();
    return w;
}

// ------------------------------------------------------------------------------------------ the batch forms' workspace and sequence
struct SbWs {                     // the workspace of one call; the last seven pieces exist in the S3DIS form only
    SbCrop* crop;
    int32_t *hist, *cnt;
    unsigned long long *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    float *dist, *pmax;
    double* pv;
    int64_t* pi;
    char* sort;
    unsigned long long *pkeys_a, *pkeys_b;
    uint32_t *pvals_a, *pvals_b;
    int64_t* perm;
    char* psort;
    int64_t *compact = nullptr, *choice = nullptr;
    unsigned long long *ckeys_a = nullptr, *ckeys_b = nullptr;
    uint32_t *cvals_a = nullptr, *cvals_b = nullptr;
    char* csort = nullptr;
    size_t bytes;
};
static SbWs sb_carve(void* workspace, int64_t n_max, int64_t k, int64_t B, bool s3dis) {
    Carve c(workspace);
    SbWs w;
    const size_t kk = (size_t)k, bk = (size_t)(B * k);
    w.crop = c.take<SbCrop>(1);
    w.hist = c.take<int32_t>(8 * 256);
    w.cnt = c.take<int32_t>(2 * (size_t)cdiv(n_max, SB_TILE));
    w.keys_a = c.take<unsigned long long>(kk);
    w.keys_b = c.take<unsigned long long>(kk);
    w.vals_a = c.take<uint32_t>(kk);
    w.vals_b = c.take<uint32_t>(kk);
    w.dist = c.take<float>(kk);
    w.pmax = c.take<float>((size_t)cdiv(k, SB_NT));
    w.pv = c.take<double>(SB_ARGMIN_BLOCKS);
    w.pi = c.take<int64_t>(SB_ARGMIN_BLOCKS);
    w.sort = c.take<char>(rsort_workspace(k));
    w.pkeys_a = c.take<unsigned long long>(bk);
    w.pkeys_b = c.take<unsigned long long>(bk);
    w.pvals_a = c.take<uint32_t>(bk);
    w.pvals_b = c.take<uint32_t>(bk);
    w.perm = c.take<int64_t>(bk);
    w.psort = c.take<char>(rsort_workspace(B * k));
    if (s3dis) {
        w.compact = c.take<int64_t>(kk);
        w.choice = c.take<int64_t>(kk);
        w.ckeys_a = c.take<unsigned long long>(2 * kk);      // the padding's sort: 2 k pairs
        w.ckeys_b = c.take<unsigned long long>(2 * kk);
        w.cvals_a = c.take<uint32_t>(2 * kk);
        w.cvals_b = c.take<uint32_t>(2 * kk);
        w.csort = c.take<char>(rsort_workspace(2 * k));
    }
    w.bytes = c.bytes();
    return w;
}

}  // namespace crf

using namespace crf;

#define SB_LAUNCH(kernel, grid, ...)                                     \
    do {                                                                 \
        hipLaunchKernelGGL(kernel, grid, blk, 0, st, __VA_ARGS__);       \
        CRF_LAUNCH_CHECK();                                              \
    } while (0)

// Both forms.  s3dis: kc = min(n, k) rows per crop on the device, padded through choice; n_min (the smallest cloud, a property of the
// table the host knows) >= k means no crop is ever padded and the padding's sort is not enqueued.
static int sb_run(bool s3dis, const crf_cloud_desc* clouds, int n_clouds, int64_t n_max, int64_t n_min, double* min_value,
                  int64_t* min_index, int64_t k, int64_t B, uint64_t seed, const int64_t* counter, double noise_scale,
                  const double* noise_in, const int64_t* perm_in, int identity_perm, const int64_t* choice_in, float* out_pos, float* out_x,
                  int x_channels, int64_t* out_y, int64_t* out_point_idx, int64_t* out_cloud_idx, double* out_center, double* noise_out,
                  int64_t* perm_out, int64_t* choice_out, void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(clouds && min_value && min_index && out_pos && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n_clouds > 0, CRF_ERR_ARG, "n_clouds=%d", n_clouds);
    CRF_REQUIRE(k > 0 && (s3dis || k <= n_max) && n_max > 0 && n_max < ((int64_t)1 << 31), CRF_ERR_ARG, "n_max=%lld k=%lld invalid",
                (long long)n_max, (long long)k);
    CRF_REQUIRE(!s3dis || (n_min > 0 && n_min <= n_max), CRF_ERR_ARG, "n_min=%lld n_max=%lld invalid", (long long)n_min, (long long)n_max);
    CRF_REQUIRE(B > 0 && B <= 65536 && B * k < ((int64_t)1 << 31) && (!s3dis || k < ((int64_t)1 << 30)), CRF_ERR_ARG, "B=%lld k=%lld invalid", (long long)B, (long long)k);
    CRF_REQUIRE(out_x == nullptr || x_channels == 3 || x_channels == 6, CRF_ERR_ARG, "x_channels=%d: 3 or 6", x_channels);
    const bool padded = s3dis && n_min < k;
    CRF_REQUIRE(counter != nullptr || (noise_in != nullptr && (perm_in != nullptr || identity_perm) && (!padded || choice_in != nullptr)),
                CRF_ERR_ARG, "a counter is needed unless noise_in, the shuffle and (with a cloud below k) the padding are given");
    CRF_REQUIRE(!(perm_in != nullptr && identity_perm), CRF_ERR_ARG, "perm_in and identity_perm exclude each other");
    const SbWs w = sb_carve(workspace, n_max, k, B, s3dis);
    CRF_REQUIRE(workspace_bytes >= w.bytes, CRF_ERR_WORKSPACE, "possibility_crop_batch workspace %zu < %zu", workspace_bytes, w.bytes);
    hipStream_t st = as_stream(stream);
    const int64_t total = B * k;
    const dim3 blk(SB_NT), one(1);
    const unsigned long long useed = (unsigned long long)seed;

    // ---- once per call: the shuffles
    const int64_t* perm = perm_in;
    if (perm_in == nullptr && !identity_perm) {
        const dim3 pgrid((unsigned)cdiv(total, SB_NT));
        SB_LAUNCH(sb_perm_keys_kernel, pgrid, useed, counter, (long long)k, (long long)total, w.pkeys_a, w.pvals_a);
        const int where = rsort_pairs_u64(w.pkeys_a, w.pvals_a, w.pkeys_b, w.pvals_b, total, 0, 64, w.psort, st);
        CRF_LAUNCH_CHECK();
        const uint32_t* sorted = where ? w.pvals_b : w.pvals_a;
        if (B > 1) {                                                   // one stable pass on the crop number: B sorted runs of k
            unsigned long long* ka = where ? w.pkeys_b : w.pkeys_a;
            unsigned long long* kb = where ? w.pkeys_a : w.pkeys_b;
            uint32_t* va = where ? w.pvals_b : w.pvals_a;
            uint32_t* vb = where ? w.pvals_a : w.pvals_b;
            SB_LAUNCH(sb_perm_crop_keys_kernel, pgrid, (const uint32_t*)va, (long long)k, (long long)total, ka);
            sorted = rsort_pairs_u64(ka, va, kb, vb, total, 0, B > 256 ? 16 : 8, w.psort, st) ? vb : va;
            CRF_LAUNCH_CHECK();
        }
        // (S3DIS form: the rows of perm_out are written per crop, cut to the crop's own row count)
        SB_LAUNCH(sb_perm_final_kernel, pgrid, sorted, (long long)k, (long long)total, w.perm, s3dis ? (int64_t*)nullptr : perm_out);
        perm = w.perm;
    } else if (perm_out != nullptr && perm_in != nullptr) {
        CRF_HIP(hipMemcpyAsync(perm_out, perm_in, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToDevice, st));
    }
    if (s3dis && choice_in != nullptr && choice_out != nullptr)
        CRF_HIP(hipMemcpyAsync(choice_out, choice_in, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToDevice, st));

    // ---- per crop
    const int64_t nb = cdiv(n_max, SB_TILE);
    const int nblk = (int)cdiv(k, SB_NT);
    const int ablocks = (int)(cdiv(n_max, SB_NT) < SB_ARGMIN_BLOCKS ? cdiv(n_max, SB_NT) : SB_ARGMIN_BLOCKS);
    const dim3 sgrid((unsigned)nb), kgrid((unsigned)nblk);
    const bool own_perm = perm == w.perm;
    int choice_bits = 32;                                              // sort key of the padding: (block j, upper hash half); j < k
    while (choice_bits < 64 && (k >> (choice_bits - 32)) != 0) choice_bits += 8;
    const auto choose_kernel = s3dis ? sb_choose_kernel<true> : sb_choose_kernel<false>;
    const auto scatter_kernel = s3dis ? sb_scatter_kernel<true> : sb_scatter_kernel<false>;
    const auto dist_kernel = s3dis ? sb_dist_kernel<true> : sb_dist_kernel<false>;
    const auto update_kernel = s3dis ? sb_update_kernel<true> : sb_update_kernel<false>;
    const SbCrop* crop = w.crop;
    for (int64_t b = 0; b < B; ++b) {
        auto row = [b, k](auto* p, int64_t width = 1) { return p ? p + b * k * width : p; };      // crop b's rows of a [B, k, width] array
        SB_LAUNCH(choose_kernel, one, clouds, n_clouds, (const double*)min_value, (const int64_t*)min_index, useed, counter, (int)b,
                  (long long)k, noise_scale, noise_in, w.crop, w.hist, noise_out, out_center, out_cloud_idx);
        for (int p = 0; p < 8; ++p) SB_LAUNCH(sb_hist_kernel, sgrid, clouds, w.crop, w.hist, p);
        SB_LAUNCH(sb_count_kernel, sgrid, clouds, w.crop, (const int32_t*)w.hist, w.cnt, (long long)nb);
        SB_LAUNCH(scatter_kernel, sgrid, clouds, crop, (const int32_t*)w.cnt, (long long)nb, (long long)k, w.keys_a, w.vals_a);
        const uint32_t* sel = rsort_pairs_u64(w.keys_a, w.vals_a, w.keys_b, w.vals_b, k, 0, 64, w.sort, st) ? w.vals_b : w.vals_a;
        CRF_LAUNCH_CHECK();
        const int64_t* choice = nullptr;
        if (s3dis) {                                                   // the padding of a short crop
            if (own_perm && (padded || perm_out != nullptr))
                SB_LAUNCH(sb_perm_compact_kernel, one, crop, row(perm), (long long)k, w.compact, row(perm_out));
            choice = row(choice_in);
            if (choice_in == nullptr && (padded || choice_out != nullptr)) {
                const uint32_t* cv = nullptr;
                if (padded) {
                    SB_LAUNCH(sb_choice_keys_kernel, dim3((unsigned)cdiv(2 * k, SB_NT)), crop, useed, counter, (int)b, (long long)k,
                              w.ckeys_a, w.cvals_a);
                    cv = rsort_pairs_u64(w.ckeys_a, w.cvals_a, w.ckeys_b, w.cvals_b, 2 * k, 0, choice_bits, w.csort, st) ? w.cvals_b : w.cvals_a;
                    CRF_LAUNCH_CHECK();
                }
                SB_LAUNCH(sb_choice_final_kernel, kgrid, crop, cv, (long long)k, w.choice, row(choice_out));
                choice = w.choice;
            }
        }
        SB_LAUNCH(dist_kernel, kgrid, clouds, crop, sel, (long long)k, w.dist, w.pmax);
        SB_LAUNCH(update_kernel, kgrid, clouds, crop, sel, row(perm), own_perm && padded ? (const int64_t*)w.compact : (const int64_t*)nullptr,
                  choice, (long long)k, (const float*)w.dist, (const float*)w.pmax, nblk, row(out_pos, 3), row(out_x, x_channels), x_channels,
                  row(out_y), row(out_point_idx));
        SB_LAUNCH(sb_argmin_partial_kernel, dim3((unsigned)ablocks), clouds, crop, w.pv, w.pi);
        SB_LAUNCH(sb_argmin_final_kernel, one, crop, (const double*)w.pv, (const int64_t*)w.pi, ablocks, min_value, min_index);
    }
    return CRF_OK;
}
#undef SB_LAUNCH

extern "C" size_t crfconv_argmin_workspace(void) { return SB_ARGMIN_BLOCKS * (sizeof(double) + sizeof(int64_t)); }

extern "C" int crfconv_argmin_f64(const double* values, int64_t n, double* out_value, int64_t* out_index,
                                  void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(values && out_value && out_index && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0, CRF_ERR_ARG, "empty array");
    CRF_REQUIRE(workspace_bytes >= crfconv_argmin_workspace(), CRF_ERR_WORKSPACE, "argmin workspace too small");
    double* pv = reinterpret_cast<double*>(workspace);
    int64_t* pi = reinterpret_cast<int64_t*>(pv + SB_ARGMIN_BLOCKS);
    int64_t blocks = cdiv(n, SB_NT);
    if (blocks > SB_ARGMIN_BLOCKS) blocks = SB_ARGMIN_BLOCKS;
    hipLaunchKernelGGL(argmin_partial_kernel, dim3((unsigned)blocks), dim3(SB_NT), 0, as_stream(stream), values, n, pv, pi);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(argmin_final_kernel, dim3(1), dim3(SB_NT), 0, as_stream(stream), pv, pi, (int)blocks, out_value,
                       out_index);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" size_t crfconv_possibility_crop_workspace(int64_t n, int64_t k) {
    if (n <= 0 || k <= 0) return 0;
    return crop_carve(nullptr, n, k).bytes;
}

extern "C" int crfconv_possibility_crop(const float* points, int64_t n, int64_t k, const int64_t* pick_index,
                                        const double* noise, const int64_t* perm, const double* point_weight,
                                        double* possibility, int64_t* out_idx, float* out_xyz, double* out_center,
                                        void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(points && pick_index && possibility && out_idx && out_xyz && workspace, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n > 0 && k > 0 && k <= n && n < ((int64_t)1 << 32), CRF_ERR_ARG, "n=%lld k=%lld invalid", (long long)n,
                (long long)k);
    const CropWs w = crop_carve(workspace, n, k);
    CRF_REQUIRE(workspace_bytes >= w.bytes, CRF_ERR_WORKSPACE, "possibility_crop workspace %zu < %zu", workspace_bytes, w.bytes);
    hipStream_t st = as_stream(stream);
    const int nblk = (int)cdiv(k, SB_NT);
    hipLaunchKernelGGL(pick_point_kernel, dim3(1), dim3(64), 0, st, points, pick_index, noise, w.center);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_keys_kernel, dim3((unsigned)cdiv(n, SB_NT)), dim3(SB_NT), 0, st, points, n, (const double*)w.center,
                       w.keys_in, w.ids_in);
    CRF_LAUNCH_CHECK();
    // stable LSD radix sort over all eight digits of the float64 keys: equal distances keep ascending point order (the KD-tree's order
    // on ties is unspecified)
    const unsigned int* sel = rsort_pairs_u64(w.keys_in, w.ids_in, w.keys_out, w.ids_out, n, 0, 64, w.sort, st) ? w.ids_out : w.ids_in;
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_dist_kernel, dim3((unsigned)nblk), dim3(SB_NT), 0, st, points, sel, k, (const double*)w.center, w.dist,
                       w.pmax);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(crop_update_kernel, dim3((unsigned)nblk), dim3(SB_NT), 0, st, points, sel, perm, k, (const double*)w.center,
                       (const float*)w.dist, (const float*)w.pmax, nblk, point_weight, possibility, out_idx, out_xyz);
    CRF_LAUNCH_CHECK();
    if (out_center) CRF_HIP(hipMemcpyAsync(out_center, w.center, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return CRF_OK;
}

extern "C" size_t crfconv_possibility_crop_batch_workspace(int64_t n_max, int64_t k, int64_t B) {
    if (n_max <= 0 || k <= 0 || B <= 0 || k > n_max) return 0;
    return sb_carve(nullptr, n_max, k, B, false).bytes;
}

extern "C" int crfconv_possibility_crop_batch(const crf_cloud_desc* clouds, int n_clouds, int64_t n_max, double* min_value,
                                              int64_t* min_index, int64_t k, int64_t B, uint64_t seed, const int64_t* counter,
                                              double noise_scale, const double* noise_in, const int64_t* perm_in, int identity_perm,
                                              float* out_pos, float* out_x, int x_channels, int64_t* out_y, int64_t* out_point_idx,
                                              int64_t* out_cloud_idx, double* out_center, double* noise_out, int64_t* perm_out,
                                              void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    return sb_run(false, clouds, n_clouds, n_max, n_max, min_value, min_index, k, B, seed, counter, noise_scale, noise_in, perm_in,
                  identity_perm, nullptr, out_pos, out_x, x_channels, out_y, out_point_idx, out_cloud_idx, out_center, noise_out, perm_out,
                  nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t crfconv_possibility_crop_batch_s3dis_workspace(int64_t n_max, int64_t k, int64_t B) {
    if (n_max <= 0 || k <= 0 || B <= 0) return 0;
    return sb_carve(nullptr, n_max, k, B, true).bytes;
}

extern "C" int crfconv_possibility_crop_batch_s3dis(const crf_cloud_desc* clouds, int n_clouds, int64_t n_max, int64_t n_min,
                                                    double* min_value, int64_t* min_index, int64_t k, int64_t B, uint64_t seed,
                                                    const int64_t* counter, double noise_scale, const double* noise_in,
                                                    const int64_t* perm_in, int identity_perm, const int64_t* choice_in, float* out_pos,
                                                    float* out_x, int x_channels, int64_t* out_y, int64_t* out_point_idx,
                                                    int64_t* out_cloud_idx, double* out_center, double* noise_out, int64_t* perm_out,
                                                    int64_t* choice_out, void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    return sb_run(true, clouds, n_clouds, n_max, n_min, min_value, min_index, k, B, seed, counter, noise_scale, noise_in, perm_in,
                  identity_perm, choice_in, out_pos, out_x, x_channels, out_y, out_point_idx, out_cloud_idx, out_center, noise_out, perm_out,
                  choice_out, workspace, workspace_bytes, stream);
}
