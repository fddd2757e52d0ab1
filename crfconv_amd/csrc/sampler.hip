// B possibility crops per call, decided and written on the device (datasets/semantic3d_dataset.py:423-460, `_get_random`, as B
// consecutive __getitem__ calls; crfconv_amd.sampling.PossibilitySampler.get_batch).  No host read anywhere, no scratch memory:
// the whole call can sit in a captured hipGraph (data.CollateGraph(sampler=)).  Bit for bit what B calls of
// crfconv_possibility_crop (evaluate.hip) give for the same jitter and shuffle, without sorting the cloud:
//
//   per crop b, in stream order (crop b + 1 sees the possibilities crop b left):
//     sb_choose_kernel   1 workgroup: cloud = arg-min of the per-cloud minima (first index on ties), seed point = that cloud's
//                        arg-min, jitter (Box-Muller in float64 on 53-bit uniforms of smp_hash, or noise_in), centre; clears the
//                        select's histograms.  The cloud is read through a DEVICE table of descriptors (crf_cloud_desc), the grids
//                        below are sized for the largest cloud and leave early beyond the chosen one.
//     sb_hist_kernel x 8 MSB-first radix SELECT on the 64-bit key (bit pattern of the float64 squared distance, recomputed from the
//                        12-byte point in every pass): pass p counts digit p of the keys that match the p digits found so far
//                        (per-wavefront LDS bins; a wavefront whose matching lanes agree on the digit -- the rule in the exponent
//                        passes -- adds one popcount; <= 256 global integer atomics per workgroup).  Every workgroup resolves the
//                        PREVIOUS pass itself (256-bin scan: the digit holding rank `want`, and the rank inside it), so there is
//                        no one-workgroup launch between the passes.  Reads 12 B per point and pass, writes nothing of size n.
//     sb_count_kernel    resolves the last digit (the k-th key is now known) and counts per tile of 4096 points the keys below it
//                        and equal to it.
//     sb_scatter_kernel  ORDER-PRESERVING compaction (ballot ranks inside a wavefront, tile bases summed from the counts): keys
//                        below the k-th in point order into [0, L), then the first k - L points with the k-th key in point order.
//     rsort_pairs_u64    the library's stable radix sort over those k pairs only: (key, point id) order, i.e. what the full stable
//                        sort of evaluate.hip yields; ties at the ball's boundary go to the lower point id.
//     sb_dist_kernel / sb_update_kernel   float32 distances, d_max, possibility += (1 - d / d_max)^2 weight -- the arithmetic of
//                        crop_dist_kernel / crop_update_kernel operation for operation -- and row b of the batch: pos (x, y
//                        centred), x = [pos, rgb], y, point_idx, through the shuffle.
//     sb_argmin_partial_kernel / sb_argmin_final_kernel   the chosen cloud's new minimum possibility (:451).
//   once per call: the B shuffles.  perm_b = stable arg-sort over t of smp_hash(seed, counter, b, 8 + t): ONE sort of the B k hashes
//   (values b k + t) followed by one stable pass on b -- the crops do not enter, so this is not repeated per crop.
//
//   S3DIS form (datasets/s3dis_dataset.py:343-379, crfconv_possibility_crop_batch_s3dis): the same select and sort for kc = min(n, k)
//   rows -- a device value; rows kc .. k of the sort's input are all-ones sentinels -- with its own distance / update kernels and the
//   padding of a short crop to k rows (further down).
// Everything is integer counting or singly rounded arithmetic in a fixed order: deterministic, no floating-point atomics.
#include <cmath>

#include "common.hpp"
#include "radix_sort.hpp"

namespace crf {

constexpr int SB_NT = 256, SB_IPT = 16, SB_TILE = SB_NT * SB_IPT;      // threads per workgroup; points per thread / per tile
constexpr int SB_ARGMIN_BLOCKS = 1024;
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
struct SbMin {
    double v;
    long long i;
};
__device__ __forceinline__ SbMin sb_min_first(SbMin a, SbMin b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ SbMin sb_wave_min(SbMin m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SbMin other;
        other.v = __shfl_xor(m.v, o, WAVE);
        other.i = __shfl_xor(m.i, o, WAVE);
        m = sb_min_first(m, other);
    }
    return m;
}

// the key of crop_keys_kernel (evaluate.hip): x then y then z, every operation singly rounded
__device__ __forceinline__ unsigned long long sb_key(const float* __restrict__ pts, long long i, double cx, double cy, double cz) {
    const double dx = (double)pts[3 * i] - cx, dy = (double)pts[3 * i + 1] - cy, dz = (double)pts[3 * i + 2] - cz;
    const double d = dadd_rn(dadd_rn(dmul_rn(dx, dx), dmul_rn(dy, dy)), dmul_rn(dz, dz));
    return (unsigned long long)__double_as_longlong(d);
}

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
    SbMin m{1.0 / 0.0, INT64_MAX};
    for (int c = lane; c < n_clouds; c += WAVE) m = sb_min_first(m, SbMin{minv[c], (long long)c});
    m = sb_wave_min(m);
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
            const unsigned long long key = sb_key(pts, i, cx, cy, cz);
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
            const unsigned long long key = sb_key(pts, i, cx, cy, cz);
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
    __shared__ int s_c[SB_NT / WAVE][2];
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
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < SB_IPT; ++r) {
        const long long i = lo + (long long)r * SB_NT + t;
        unsigned long long key = ~0ull;
        if (i < n) key = sb_key(pts, i, cx, cy, cz);
        const bool less = i < n && key < kth, eq = i < n && key == kth;
        const unsigned long long ml = __ballot(less), me = __ballot(eq);
        if (lane == 0) { s_c[wave][0] = __popcll(ml); s_c[wave][1] = __popcll(me); }
        __syncthreads();
        long long sl = bl, se = be;
        int tl = 0, te = 0;
#pragma unroll
        for (int w = 0; w < SB_NT / WAVE; ++w) {
            if (w < wave) { sl += s_c[w][0]; se += s_c[w][1]; }
            tl += s_c[w][0];
            te += s_c[w][1];
        }
        if (less) {
            const long long slot = sl + __popcll(ml & lt);
            if (slot < L) { keys_out[slot] = key; vals_out[slot] = (uint32_t)i; }
        } else if (eq) {
            const long long e = se + __popcll(me & lt);
            if (e < want) { keys_out[L + e] = key; vals_out[L + e] = (uint32_t)i; }
        }
        bl += tl;
        be += te;
        __syncthreads();
    }
}

// crop_dist_kernel of evaluate.hip, the cloud taken from the crop's descriptor
__global__ __launch_bounds__(SB_NT) void sb_dist_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                        const uint32_t* __restrict__ sel, long long k, float* __restrict__ dist,
                                                        float* __restrict__ pmax) {
    __shared__ float s_red[SB_NT / WAVE];
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    const float* __restrict__ points = clouds[st->cloud].points;
    float d = 0.f;
    if (t < k) {
        const long long i = sel[t];
        if (i < st->n) {
            const double dx = (double)points[3 * i] - st->center[0], dy = (double)points[3 * i + 1] - st->center[1],
                         dz = (double)points[3 * i + 2] - st->center[2];
            d = add_rn(add_rn((float)dmul_rn(dx, dx), (float)dmul_rn(dy, dy)), (float)dmul_rn(dz, dz));
        }
        dist[t] = d;
    }
    float mx = d;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SB_NT / WAVE; ++w) mx = fmaxf(mx, s_red[w]);
        pmax[blockIdx.x] = mx;
    }
}

// crop_update_kernel of evaluate.hip + the gathers of labels and colours, into row b of the batch
__global__ __launch_bounds__(SB_NT) void sb_update_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                          const uint32_t* __restrict__ sel, const int64_t* __restrict__ perm, long long k,
                                                          const float* __restrict__ dist, const float* __restrict__ pmax, int nblk,
                                                          float* __restrict__ out_pos, float* __restrict__ out_x, int xc,
                                                          int64_t* __restrict__ out_y, int64_t* __restrict__ out_idx) {
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (t >= k) return;
    const crf_cloud_desc cd = clouds[st->cloud];
    float dmax = pmax[0];
    for (int b = 1; b < nblk; ++b) dmax = fmaxf(dmax, pmax[b]);
    const long long src = perm ? perm[t] : t;               // output row t shows selected element perm[t] (the shuffle)
    if (src < 0 || src >= k) return;
    const long long i = sel[src];
    if (i >= cd.n) return;
    const float u = sub_rn(1.0f, __fdiv_rn(dist[src], dmax));
    const float sq = mul_rn(u, u);
    const double delta = cd.point_weight ? dmul_rn((double)sq, cd.point_weight[i]) : (double)sq;
    cd.possibility[i] += delta;                              // rows of a crop are distinct points
    const float px = (float)((double)cd.points[3 * i + 0] - st->center[0]);
    const float py = (float)((double)cd.points[3 * i + 1] - st->center[1]);
    const float pz = cd.points[3 * i + 2];
    out_pos[3 * t + 0] = px;
    out_pos[3 * t + 1] = py;
    out_pos[3 * t + 2] = pz;
    if (out_x != nullptr) {
        float* xr = out_x + (size_t)t * xc;
        xr[0] = px; xr[1] = py; xr[2] = pz;
        if (xc == 6) {
            xr[3] = cd.rgb ? cd.rgb[3 * i + 0] : 0.f;
            xr[4] = cd.rgb ? cd.rgb[3 * i + 1] : 0.f;
            xr[5] = cd.rgb ? cd.rgb[3 * i + 2] : 0.f;
        }
    }
    if (out_y != nullptr) out_y[t] = cd.labels ? cd.labels[i] : 0;
    if (out_idx != nullptr) out_idx[t] = i;
}

__global__ __launch_bounds__(SB_NT) void sb_argmin_partial_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                                  double* __restrict__ pv, int64_t* __restrict__ pi) {
    __shared__ double s_v[SB_NT / WAVE];
    __shared__ long long s_i[SB_NT / WAVE];
    const double* __restrict__ v = clouds[st->cloud].possibility;
    const long long n = st->n;
    SbMin m{1.0 / 0.0, INT64_MAX};
    for (long long i = (long long)blockIdx.x * SB_NT + threadIdx.x; i < n; i += (long long)gridDim.x * SB_NT)
        m = sb_min_first(m, SbMin{v[i], i});
    m = sb_wave_min(m);
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = m.v; s_i[threadIdx.x >> 6] = m.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SB_NT / WAVE; ++w) m = sb_min_first(m, SbMin{s_v[w], s_i[w]});
        pv[blockIdx.x] = m.v;
        pi[blockIdx.x] = m.i;
    }
}
__global__ __launch_bounds__(SB_NT) void sb_argmin_final_kernel(const SbCrop* __restrict__ st, const double* __restrict__ pv,
                                                                const int64_t* __restrict__ pi, int nblk, double* __restrict__ minv,
                                                                int64_t* __restrict__ mini) {
    __shared__ double s_v[SB_NT / WAVE];
    __shared__ long long s_i[SB_NT / WAVE];
    SbMin m{1.0 / 0.0, INT64_MAX};
    for (int b = threadIdx.x; b < nblk; b += SB_NT) m = sb_min_first(m, SbMin{pv[b], (long long)pi[b]});
    m = sb_wave_min(m);
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = m.v; s_i[threadIdx.x >> 6] = m.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SB_NT / WAVE; ++w) m = sb_min_first(m, SbMin{s_v[w], s_i[w]});
        minv[st->cloud] = m.v;
        mini[st->cloud] = m.i;
    }
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

// ---- the S3DIS form (datasets/s3dis_dataset.py:343-379): all three axes centred, float32 distances of the float32 centred
// coordinates, weight 1, a room smaller than k taken whole (kc = n rows) and padded to k rows by `choice`.
constexpr unsigned long long SMP_CHOICE_SLOT = 1ull << 32;             // slot (j + 1) 2^32 + t: padding key of element t of block j

// np.sum(np.square(query_xyz.astype(np.float32)), axis=1) (:363): x x + y y + z z in float32, every operation rounded once
__global__ __launch_bounds__(SB_NT) void sb_dist_s3dis_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                              const uint32_t* __restrict__ sel, long long k, float* __restrict__ dist,
                                                              float* __restrict__ pmax) {
    __shared__ float s_red[SB_NT / WAVE];
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    const float* __restrict__ points = clouds[st->cloud].points;
    float d = 0.f;
    if (t < k) {
        const long long i = sel[t];
        if (t < st->kc && i < st->n) {
            const float px = (float)((double)points[3 * i] - st->center[0]), py = (float)((double)points[3 * i + 1] - st->center[1]),
                        pz = (float)((double)points[3 * i + 2] - st->center[2]);
            d = add_rn(add_rn(mul_rn(px, px), mul_rn(py, py)), mul_rn(pz, pz));
        }
        dist[t] = d;
    }
    float mx = d;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SB_NT / WAVE; ++w) mx = fmaxf(mx, s_red[w]);
        pmax[blockIdx.x] = mx;
    }
}

// possibility[query_idx] += (1 - d / d_max)^2 over the kc DISTINCT rows of the crop (:364-365), then row t of the batch = row
// choice[t] of the shuffled crop = selected element perm[choice[t]] (:357, :375-377).  kc == k: choice is the identity.
__global__ __launch_bounds__(SB_NT) void sb_update_s3dis_kernel(const crf_cloud_desc* __restrict__ clouds, const SbCrop* __restrict__ st,
                                                                const uint32_t* __restrict__ sel, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ perm_compact,
                                                                const int64_t* __restrict__ choice, long long k,
                                                                const float* __restrict__ dist, const float* __restrict__ pmax, int nblk,
                                                                float* __restrict__ out_pos, float* __restrict__ out_x, int xc,
                                                                int64_t* __restrict__ out_y, int64_t* __restrict__ out_idx) {
    const long long t = (long long)blockIdx.x * SB_NT + threadIdx.x;
    if (t >= k) return;
    const crf_cloud_desc cd = clouds[st->cloud];
    const long long kc = st->kc;
    if (t < kc) {
        float dmax = pmax[0];
        for (int b = 1; b < nblk; ++b) dmax = fmaxf(dmax, pmax[b]);
        const long long j = sel[t];
        if (j < cd.n) {
            const float u = sub_rn(1.0f, __fdiv_rn(dist[t], dmax));
            cd.possibility[j] += (double)mul_rn(u, u);              // the kc selected rows are distinct points
        }
    }
    long long s = t;
    if (kc < k) {
        if (choice == nullptr) return;
        s = choice[t];
    }
    if (s < 0 || s >= kc) return;
    if (kc < k && perm_compact != nullptr) perm = perm_compact;     // the device's own shuffle, restricted to kc rows
    const long long src = perm ? perm[s] : s;
    if (src < 0 || src >= kc) return;
    const long long i = sel[src];
    if (i >= cd.n) return;
    const float px = (float)((double)cd.points[3 * i + 0] - st->center[0]);
    const float py = (float)((double)cd.points[3 * i + 1] - st->center[1]);
    const float pz = (float)((double)cd.points[3 * i + 2] - st->center[2]);
    out_pos[3 * t + 0] = px;
    out_pos[3 * t + 1] = py;
    out_pos[3 * t + 2] = pz;
    if (out_x != nullptr) {
        float* xr = out_x + (size_t)t * xc;
        xr[0] = px; xr[1] = py; xr[2] = pz;
        if (xc == 6) {
            xr[3] = cd.rgb ? cd.rgb[3 * i + 0] : 0.f;
            xr[4] = cd.rgb ? cd.rgb[3 * i + 1] : 0.f;
            xr[5] = cd.rgb ? cd.rgb[3 * i + 2] : 0.f;
        }
    }
    if (out_y != nullptr) out_y[t] = cd.labels ? cd.labels[i] : 0;
    if (out_idx != nullptr) out_idx[t] = i;
}

// The shuffle of a crop of kc < k rows: the stable ranking of the first kc hashes of row b = the entries below kc of the row's full
// arg-sort, in their order.  One workgroup, order-preserving compaction; perm_out (or NULL) <- the kc entries, then -1.
__global__ __launch_bounds__(SB_NT) void sb_perm_compact_kernel(const SbCrop* __restrict__ st, const int64_t* __restrict__ full, long long k,
                                                                int64_t* __restrict__ compact, int64_t* __restrict__ perm_out) {
    __shared__ int s_c[SB_NT / WAVE];
    const long long kc = st->kc;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
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
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_c[wave] = __popcll(m);
        __syncthreads();
        long long slot = base;
        int total = 0;
#pragma unroll
        for (int w = 0; w < SB_NT / WAVE; ++w) {
            if (w < wave) slot += s_c[w];
            total += s_c[w];
        }
        if (keep) {
            slot += __popcll(m & ((1ull << lane) - 1ull));
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

static size_t sb_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct SbLayout {
    size_t crop, hist, cnt, keys_a, keys_b, vals_a, vals_b, dist, pmax, pv, pi, sort, pkeys_a, pkeys_b, pvals_a, pvals_b, perm, psort, total;
    size_t compact, choice, ckeys_a, ckeys_b, cvals_a, cvals_b, csort;      // the S3DIS form only
};
static SbLayout sb_layout(int64_t n_max, int64_t k, int64_t B, bool s3dis = false) {
    SbLayout l;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += sb_align(bytes); return at; };
    const size_t nb = (size_t)cdiv(n_max, SB_TILE), kk = (size_t)k, bk = (size_t)(B * k);
    l.crop = take(sizeof(SbCrop));
    l.hist = take(8 * 256 * sizeof(int32_t));
    l.cnt = take(2 * nb * sizeof(int32_t));
    l.keys_a = take(8 * kk);
    l.keys_b = take(8 * kk);
    l.vals_a = take(4 * kk);
    l.vals_b = take(4 * kk);
    l.dist = take(4 * kk);
    l.pmax = take(4 * (size_t)cdiv(k, SB_NT));
    l.pv = take(8 * SB_ARGMIN_BLOCKS);
    l.pi = take(8 * SB_ARGMIN_BLOCKS);
    l.sort = take(rsort_workspace(k));
    l.pkeys_a = take(8 * bk);
    l.pkeys_b = take(8 * bk);
    l.pvals_a = take(4 * bk);
    l.pvals_b = take(4 * bk);
    l.perm = take(8 * bk);
    l.psort = take(rsort_workspace(B * k));
    l.compact = l.choice = l.ckeys_a = l.ckeys_b = l.cvals_a = l.cvals_b = l.csort = 0;
    if (s3dis) {
        l.compact = take(8 * kk);
        l.choice = take(8 * kk);
        l.ckeys_a = take(16 * kk);
        l.ckeys_b = take(16 * kk);
        l.cvals_a = take(8 * kk);
        l.cvals_b = take(8 * kk);
        l.csort = take(rsort_workspace(2 * k));
    }
    l.total = o + 256;                                                 // (room to align the caller's pointer)
    return l;
}

}  // namespace crf

using namespace crf;

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
    const size_t need = sb_layout(n_max, k, B, s3dis).total;
    CRF_REQUIRE(workspace_bytes >= need, CRF_ERR_WORKSPACE, "possibility_crop_batch workspace %zu < %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const SbLayout l = sb_layout(n_max, k, B, s3dis);
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    auto at = [ws](size_t off) { return ws + off; };
    auto* crop = reinterpret_cast<SbCrop*>(at(l.crop));
    auto* hist = reinterpret_cast<int32_t*>(at(l.hist));
    auto* cnt = reinterpret_cast<int32_t*>(at(l.cnt));
    auto* keys_a = reinterpret_cast<unsigned long long*>(at(l.keys_a));
    auto* keys_b = reinterpret_cast<unsigned long long*>(at(l.keys_b));
    auto* vals_a = reinterpret_cast<uint32_t*>(at(l.vals_a));
    auto* vals_b = reinterpret_cast<uint32_t*>(at(l.vals_b));
    auto* dist = reinterpret_cast<float*>(at(l.dist));
    auto* pmax = reinterpret_cast<float*>(at(l.pmax));
    auto* pv = reinterpret_cast<double*>(at(l.pv));
    auto* pi = reinterpret_cast<int64_t*>(at(l.pi));
    auto* pkeys_a = reinterpret_cast<unsigned long long*>(at(l.pkeys_a));
    auto* pkeys_b = reinterpret_cast<unsigned long long*>(at(l.pkeys_b));
    auto* pvals_a = reinterpret_cast<uint32_t*>(at(l.pvals_a));
    auto* pvals_b = reinterpret_cast<uint32_t*>(at(l.pvals_b));
    auto* perm_ws = reinterpret_cast<int64_t*>(at(l.perm));

    const int64_t total = B * k;
    const dim3 blk(SB_NT);
    const int64_t* perm = perm_in;
    if (perm_in == nullptr && !identity_perm) {
        const dim3 pgrid((unsigned)cdiv(total, SB_NT));
        hipLaunchKernelGGL(sb_perm_keys_kernel, pgrid, blk, 0, st, (unsigned long long)seed, counter, (long long)k, (long long)total,
                           pkeys_a, pvals_a);
        CRF_LAUNCH_CHECK();
        int where = rsort_pairs_u64(pkeys_a, pvals_a, pkeys_b, pvals_b, total, 0, 64, at(l.psort), st);
        CRF_LAUNCH_CHECK();
        if (B > 1) {                                                   // one stable pass on the crop number: B sorted runs of k
            unsigned long long* ka = where ? pkeys_b : pkeys_a;
            unsigned long long* kb = where ? pkeys_a : pkeys_b;
            uint32_t* va = where ? pvals_b : pvals_a;
            uint32_t* vb = where ? pvals_a : pvals_b;
            hipLaunchKernelGGL(sb_perm_crop_keys_kernel, pgrid, blk, 0, st, va, (long long)k, (long long)total, ka);
            CRF_LAUNCH_CHECK();
            const int w2 = rsort_pairs_u64(ka, va, kb, vb, total, 0, B > 256 ? 16 : 8, at(l.psort), st);
            CRF_LAUNCH_CHECK();
            pvals_a = w2 ? vb : va;
        } else if (where) {
            pvals_a = pvals_b;
        }
        // (S3DIS form: the rows of perm_out are written per crop, cut to the crop's own row count)
        hipLaunchKernelGGL(sb_perm_final_kernel, pgrid, blk, 0, st, pvals_a, (long long)k, (long long)total, perm_ws,
                           s3dis ? (int64_t*)nullptr : perm_out);
        CRF_LAUNCH_CHECK();
        perm = perm_ws;
    } else if (perm_out != nullptr && perm_in != nullptr) {
        CRF_HIP(hipMemcpyAsync(perm_out, perm_in, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToDevice, st));
    }

    const int64_t nb = cdiv(n_max, SB_TILE);
    const int nblk = (int)cdiv(k, SB_NT);
    int64_t ablocks = cdiv(n_max, SB_NT);
    if (ablocks > SB_ARGMIN_BLOCKS) ablocks = SB_ARGMIN_BLOCKS;
    const dim3 sgrid((unsigned)nb), kgrid((unsigned)nblk);
    auto* compact = reinterpret_cast<int64_t*>(at(l.compact));
    auto* choice_ws = reinterpret_cast<int64_t*>(at(l.choice));
    const bool own_perm = perm == perm_ws;
    int choice_bits = 32;                                              // sort key of the padding: (block j, upper hash half); j < k
    while (choice_bits < 64 && (k >> (choice_bits - 32)) != 0) choice_bits += 8;
    if (s3dis && choice_in != nullptr && choice_out != nullptr)
        CRF_HIP(hipMemcpyAsync(choice_out, choice_in, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToDevice, st));
    for (int64_t b = 0; b < B; ++b) {
        if (s3dis) {
            hipLaunchKernelGGL(sb_choose_kernel<true>, dim3(1), blk, 0, st, clouds, n_clouds, (const double*)min_value,
                               (const int64_t*)min_index, (unsigned long long)seed, counter, (int)b, (long long)k, noise_scale, noise_in,
                               crop, hist, noise_out, out_center, out_cloud_idx);
            CRF_LAUNCH_CHECK();
            for (int p = 0; p < 8; ++p) {
                hipLaunchKernelGGL(sb_hist_kernel, sgrid, blk, 0, st, clouds, crop, hist, p);
                CRF_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(sb_count_kernel, sgrid, blk, 0, st, clouds, crop, (const int32_t*)hist, cnt, (long long)nb);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(sb_scatter_kernel<true>, sgrid, blk, 0, st, clouds, (const SbCrop*)crop, (const int32_t*)cnt, (long long)nb,
                               (long long)k, keys_a, vals_a);
            CRF_LAUNCH_CHECK();
            const uint32_t* sel = rsort_pairs_u64(keys_a, vals_a, keys_b, vals_b, k, 0, 64, at(l.sort), st) ? vals_b : vals_a;
            CRF_LAUNCH_CHECK();
            if (own_perm && (padded || perm_out != nullptr)) {
                hipLaunchKernelGGL(sb_perm_compact_kernel, dim3(1), blk, 0, st, (const SbCrop*)crop, perm + b * k, (long long)k, compact,
                                   perm_out ? perm_out + b * k : (int64_t*)nullptr);
                CRF_LAUNCH_CHECK();
            }
            const int64_t* choice = choice_in ? choice_in + b * k : (const int64_t*)nullptr;
            if (choice_in == nullptr && (padded || choice_out != nullptr)) {
                const uint32_t* cv = nullptr;
                if (padded) {
                    auto* cka = reinterpret_cast<unsigned long long*>(at(l.ckeys_a));
                    auto* ckb = reinterpret_cast<unsigned long long*>(at(l.ckeys_b));
                    auto* cva = reinterpret_cast<uint32_t*>(at(l.cvals_a));
                    auto* cvb = reinterpret_cast<uint32_t*>(at(l.cvals_b));
                    hipLaunchKernelGGL(sb_choice_keys_kernel, dim3((unsigned)cdiv(2 * k, SB_NT)), blk, 0, st, (const SbCrop*)crop,
                                       (unsigned long long)seed, counter, (int)b, (long long)k, cka, cva);
                    CRF_LAUNCH_CHECK();
                    cv = rsort_pairs_u64(cka, cva, ckb, cvb, 2 * k, 0, choice_bits, at(l.csort), st) ? cvb : cva;
                    CRF_LAUNCH_CHECK();
                }
                hipLaunchKernelGGL(sb_choice_final_kernel, kgrid, blk, 0, st, (const SbCrop*)crop, cv, (long long)k, choice_ws,
                                   choice_out ? choice_out + b * k : (int64_t*)nullptr);
                CRF_LAUNCH_CHECK();
                choice = choice_ws;
            }
            hipLaunchKernelGGL(sb_dist_s3dis_kernel, kgrid, blk, 0, st, clouds, (const SbCrop*)crop, sel, (long long)k, dist, pmax);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(sb_update_s3dis_kernel, kgrid, blk, 0, st, clouds, (const SbCrop*)crop, sel,
                               perm ? perm + b * k : (const int64_t*)nullptr, own_perm && padded ? (const int64_t*)compact : (const int64_t*)nullptr,
                               choice, (long long)k, (const float*)dist, (const float*)pmax, nblk, out_pos + (size_t)b * k * 3,
                               out_x ? out_x + (size_t)b * k * x_channels : (float*)nullptr, x_channels,
                               out_y ? out_y + b * k : (int64_t*)nullptr, out_point_idx ? out_point_idx + b * k : (int64_t*)nullptr);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(sb_argmin_partial_kernel, dim3((unsigned)ablocks), blk, 0, st, clouds, (const SbCrop*)crop, pv, pi);
            CRF_LAUNCH_CHECK();
            hipLaunchKernelGGL(sb_argmin_final_kernel, dim3(1), blk, 0, st, (const SbCrop*)crop, (const double*)pv, (const int64_t*)pi,
                               (int)ablocks, min_value, min_index);
            CRF_LAUNCH_CHECK();
            continue;
        }
        hipLaunchKernelGGL(sb_choose_kernel<false>, dim3(1), blk, 0, st, clouds, n_clouds, (const double*)min_value, (const int64_t*)min_index,
                           (unsigned long long)seed, counter, (int)b, (long long)k, noise_scale, noise_in, crop, hist, noise_out,
                           out_center, out_cloud_idx);
        CRF_LAUNCH_CHECK();
        for (int p = 0; p < 8; ++p) {
            hipLaunchKernelGGL(sb_hist_kernel, sgrid, blk, 0, st, clouds, crop, hist, p);
            CRF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sb_count_kernel, sgrid, blk, 0, st, clouds, crop, (const int32_t*)hist, cnt, (long long)nb);
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_scatter_kernel<false>, sgrid, blk, 0, st, clouds, (const SbCrop*)crop, (const int32_t*)cnt, (long long)nb,
                           (long long)k, keys_a, vals_a);
        CRF_LAUNCH_CHECK();
        const uint32_t* sel = rsort_pairs_u64(keys_a, vals_a, keys_b, vals_b, k, 0, 64, at(l.sort), st) ? vals_b : vals_a;
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_dist_kernel, kgrid, blk, 0, st, clouds, (const SbCrop*)crop, sel, (long long)k, dist, pmax);
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_update_kernel, kgrid, blk, 0, st, clouds, (const SbCrop*)crop, sel,
                           perm ? perm + b * k : (const int64_t*)nullptr, (long long)k, (const float*)dist, (const float*)pmax, nblk,
                           out_pos + (size_t)b * k * 3, out_x ? out_x + (size_t)b * k * x_channels : (float*)nullptr, x_channels,
                           out_y ? out_y + b * k : (int64_t*)nullptr, out_point_idx ? out_point_idx + b * k : (int64_t*)nullptr);
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_argmin_partial_kernel, dim3((unsigned)ablocks), blk, 0, st, clouds, (const SbCrop*)crop, pv, pi);
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_argmin_final_kernel, dim3(1), blk, 0, st, (const SbCrop*)crop, (const double*)pv, (const int64_t*)pi,
                           (int)ablocks, min_value, min_index);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

extern "C" size_t crfconv_possibility_crop_batch_workspace(int64_t n_max, int64_t k, int64_t B) {
    if (n_max <= 0 || k <= 0 || B <= 0 || k > n_max) return 0;
    return sb_layout(n_max, k, B).total;
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
    return sb_layout(n_max, k, B, true).total;
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
