// The transforms ahead of the sparse networks on a RAGGED batch, in place: pos [N, 3] (+ norm [N, 3], + x [N, C]) and a device
// int64 ptr [S + 1] (cloud b = rows ptr[b] .. ptr[b + 1]).  Per cloud, every step optional, in this order:
//   center     pos -= c, c = the cloud's mean: summed in double, a thread over its own points in ascending local index, then a
//              fixed tree over the workgroup; rounded ONCE to float32
//   normalize  pos *= k, k = (1 / max |pos|) * 0.999999f over the centred cloud (PyG NormalizeScale); a cloud whose maximum is 0
//              (one point, coincident points) keeps its zeros: k = 0 (PyG writes NaN there)
//   rotate, scale, flip, noise, drop   the draws, laws and singly rounded instruction sequences of augment.hip
//              (augment_common.hpp); the hash's cloud index is the cloud's position in ptr, the noise hash's point index the LOCAL row
//   normals    rotate n <- n @ M; scale n_i <- n_i / s_i, then renormalised to unit length (a zero normal stays zero); flip of
//              axis i n_i <- -n_i; center, normalize and noise leave them alone
//   x          x[:, 0:3] <- pos; x[:, 3:6] <- norm in the [pos, norm] layout, x[:, 3:6] <- 0 on a dropped rgb in the [pos, rgb] one
//
// aug_segments_kernel: ONE launch, one 1024-thread workgroup per cloud, grid = S.  The passes -- mean, max |p - c|, the per-axis
// max of the rotated and scaled coordinate (only when an axis may flip), apply -- are separated by workgroup barriers only: no grid
// barrier, no atomics, no workspace, nothing to zero; bitwise deterministic and capturable.  A lane owns four consecutive LOCAL
// rows per trip (12 floats of pos), so every reduction order is a function of the local index and a cloud's output does not depend
// on its neighbours in the batch.  A cloud starts at an arbitrary row: the lane's 12 floats start at any dword, so they move as up
// to 3 head dwords, the 16-byte vectors from the first 16-byte aligned address on, and the tail dwords (seg_ld / seg_st); a partial
// group of rows moves per dword.  A cloud of at most 4096 points keeps its rows in registers between the passes; a larger one is
// walked once per pass.
//
// fixed_points_kernel: PyG FixedPoints per cloud, one workgroup per cloud, one launch: see the comment above it.
#include "augment_common.hpp"

namespace crf {

constexpr int SEG_NT = 1024, SEG_PPT = 4, SEG_PPB = SEG_NT * SEG_PPT, SEG_NW = SEG_NT / WAVE;

// NF consecutive floats at p (4-byte aligned), H = dwords in front of the first 16-byte aligned address
template <int NF, int H>
__device__ __forceinline__ void seg_ld_h(const float* __restrict__ p, float (&v)[NF]) {
    constexpr int NV = (NF - H) / 4;
#pragma unroll
    for (int j = 0; j < H; ++j) v[j] = p[j];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const float4 w = ld4(p + H + 4 * q);
        v[H + 4 * q] = w.x; v[H + 4 * q + 1] = w.y; v[H + 4 * q + 2] = w.z; v[H + 4 * q + 3] = w.w;
    }
#pragma unroll
    for (int j = H + 4 * NV; j < NF; ++j) v[j] = p[j];
}
template <int NF, int H>
__device__ __forceinline__ void seg_st_h(float* __restrict__ p, const float (&v)[NF]) {
    constexpr int NV = (NF - H) / 4;
#pragma unroll
    for (int j = 0; j < H; ++j) p[j] = v[j];
#pragma unroll
    for (int q = 0; q < NV; ++q) st4(p + H + 4 * q, make_float4(v[H + 4 * q], v[H + 4 * q + 1], v[H + 4 * q + 2], v[H + 4 * q + 3]));
#pragma unroll
    for (int j = H + 4 * NV; j < NF; ++j) p[j] = v[j];
}
__device__ __forceinline__ int seg_head(const float* p) { return (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u); }

// the lane's rows [r0, r0 + 4) of a [.., 3] array, nv of them inside the cloud
__device__ __forceinline__ void seg_ld12(const float* __restrict__ p, int nv, float (&v)[12]) {
    if (nv == SEG_PPT) {
        switch (seg_head(p)) {                                   // (the same for every full group of a cloud)
            case 0: seg_ld_h<12, 0>(p, v); break;
            case 1: seg_ld_h<12, 1>(p, v); break;
            case 2: seg_ld_h<12, 2>(p, v); break;
            default: seg_ld_h<12, 3>(p, v); break;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < 3 * nv ? p[j] : 0.f;
    }
}
__device__ __forceinline__ void seg_st12(float* __restrict__ p, int nv, const float (&v)[12]) {
    if (nv == SEG_PPT) {
        switch (seg_head(p)) {
            case 0: seg_st_h<12, 0>(p, v); break;
            case 1: seg_st_h<12, 1>(p, v); break;
            case 2: seg_st_h<12, 2>(p, v); break;
            default: seg_st_h<12, 3>(p, v); break;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * nv) p[j] = v[j];
    }
}

// max over the workgroup of three values (-inf = nothing); every thread receives them.  s_red [3 * SEG_NW]
__device__ __forceinline__ void seg_block_max3(float& m0, float& m1, float& m2, float* s_red) {
    m0 = group_max<WAVE>(m0);
    m1 = group_max<WAVE>(m1);
    m2 = group_max<WAVE>(m2);
    const int w = threadIdx.x / WAVE;
    __syncthreads();                                             // (the previous use of s_red has been read)
    if ((threadIdx.x & (WAVE - 1)) == 0) { s_red[3 * w] = m0; s_red[3 * w + 1] = m1; s_red[3 * w + 2] = m2; }
    __syncthreads();
    m0 = s_red[0]; m1 = s_red[1]; m2 = s_red[2];
#pragma unroll
    for (int k = 1; k < SEG_NW; ++k) {
        m0 = fmaxf(m0, s_red[3 * k]); m1 = fmaxf(m1, s_red[3 * k + 1]); m2 = fmaxf(m2, s_red[3 * k + 2]);
    }
}

// a fixed tree: the xor butterfly inside a wavefront (a + b == b + a bit for bit: every lane holds the same sum), then the
// wavefronts' sums in ascending order
__device__ __forceinline__ double seg_block_sum(double v, double* s_sum) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = dadd_rn(v, __shfl_xor(v, o, WAVE));
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) s_sum[threadIdx.x / WAVE] = v;
    __syncthreads();
    double t = s_sum[0];
#pragma unroll
    for (int k = 1; k < SEG_NW; ++k) t = dadd_rn(t, s_sum[k]);
    return t;
}

// center and normalize of one coordinate: ONE instruction sequence for every pass
__device__ __forceinline__ float seg_center(const crf_augment_segments_spec& sp, float p, float c) { return sp.center ? sub_rn(p, c) : p; }

__global__ __launch_bounds__(SEG_NT) void aug_segments_kernel(float* __restrict__ pos, float* __restrict__ norm, float* __restrict__ x,
                                                             long long N, int C, const long long* __restrict__ ptr,
                                                             const crf_augment_segments_spec sp, unsigned long long seed,
                                                             const long long* __restrict__ counter,
                                                             const float* __restrict__ params_in, const float* __restrict__ noise_in,
                                                             float* __restrict__ params_out, float* __restrict__ stats_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    // the cloud's rows, kept inside [0, N] whatever ptr holds
    long long r_lo = ptr[b], r_hi = ptr[b + 1];
    r_lo = r_lo < 0 ? 0 : (r_lo > N ? N : r_lo);
    r_hi = r_hi < r_lo ? r_lo : (r_hi > N ? N : r_hi);
    const long long n = r_hi - r_lo;
    const long long trips = (n + SEG_PPB - 1) / SEG_PPB;
    const bool resident = n <= SEG_PPB;                          // one trip: the lane's rows stay in registers between the passes
    float* const cpos = pos + 3 * r_lo;

    float v[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = 0.f;                     // (a lane without rows in a trip still runs the passes' arithmetic)
    auto rows_of = [&](long long trip, long long& l0) -> int {   // the lane's local rows [l0, l0 + nv) of this trip
        l0 = (trip * SEG_NT + tid) * SEG_PPT;
        const long long left = n - l0;
        return left <= 0 ? 0 : (left < SEG_PPT ? (int)left : SEG_PPT);
    };
    if (resident) {
        long long l0;
        const int nv = rows_of(0, l0);
        if (nv > 0) seg_ld12(cpos + 3 * l0, nv, v);
    }
    const unsigned long long ctr = (unsigned long long)counter[0];
    const AugParams P = aug_cloud_params(sp, seed, ctr, b, params_in);

    __shared__ double s_sum[SEG_NW];
    __shared__ float s_red[3 * SEG_NW];

    // ---- pass 1: the mean
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (sp.center) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (long long trip = 0; trip < trips; ++trip) {
            long long l0;
            const int nv = rows_of(trip, l0);
            if (!resident && nv > 0) seg_ld12(cpos + 3 * l0, nv, v);
#pragma unroll
            for (int j = 0; j < SEG_PPT; ++j)
                if (j < nv) { a0 = dadd_rn(a0, (double)v[3 * j]); a1 = dadd_rn(a1, (double)v[3 * j + 1]); a2 = dadd_rn(a2, (double)v[3 * j + 2]); }
        }
        a0 = seg_block_sum(a0, s_sum);
        a1 = seg_block_sum(a1, s_sum);
        a2 = seg_block_sum(a2, s_sum);
        if (n > 0) { c0 = (float)(a0 / (double)n); c1 = (float)(a1 / (double)n); c2 = (float)(a2 / (double)n); }
    }
    // ---- pass 2: max |p - c|
    float k = 1.f;
    if (sp.normalize) {
        float m = -INFINITY;
        for (long long trip = 0; trip < trips; ++trip) {
            long long l0;
            const int nv = rows_of(trip, l0);
            if (!resident && nv > 0) seg_ld12(cpos + 3 * l0, nv, v);
#pragma unroll
            for (int j = 0; j < SEG_PPT; ++j)
                if (j < nv)
                    m = fmaxf(m, fmaxf(fabsf(seg_center(sp, v[3 * j], c0)), fmaxf(fabsf(seg_center(sp, v[3 * j + 1], c1)),
                                                                                 fabsf(seg_center(sp, v[3 * j + 2], c2)))));
        }
        float m1 = m, m2 = m;
        seg_block_max3(m, m1, m2, s_red);
        k = m > 0.f ? mul_rn(1.f / m, 0.999999f) : 0.f;          // (no point, or a maximum of 0: the zeros stay)
    }
    auto place = [&](float& px, float& py, float& pz) {          // center, normalize, rotate, scale: the same in passes 3 and 4
        px = seg_center(sp, px, c0); py = seg_center(sp, py, c1); pz = seg_center(sp, pz, c2);
        if (sp.normalize) { px = mul_rn(px, k); py = mul_rn(py, k); pz = mul_rn(pz, k); }
        aug_rotate_scale(sp, P, px, py, pz);
    };
    // ---- pass 3: the per-axis max of the placed coordinate, when an axis may flip (sp.flip_axes: uniform over the grid)
    float cm0 = 0.f, cm1 = 0.f, cm2 = 0.f;
    if (sp.flip_axes != 0) {
        cm0 = cm1 = cm2 = -INFINITY;
        for (long long trip = 0; trip < trips; ++trip) {
            long long l0;
            const int nv = rows_of(trip, l0);
            if (!resident && nv > 0) seg_ld12(cpos + 3 * l0, nv, v);
#pragma unroll
            for (int j = 0; j < SEG_PPT; ++j) {
                float px = v[3 * j], py = v[3 * j + 1], pz = v[3 * j + 2];
                place(px, py, pz);
                if (j < nv) { cm0 = fmaxf(cm0, px); cm1 = fmaxf(cm1, py); cm2 = fmaxf(cm2, pz); }
            }
        }
        seg_block_max3(cm0, cm1, cm2, s_red);
    }
    if (tid == 0) {
        if (params_out != nullptr) aug_write_params(params_out + (size_t)b * 8, P, cm0, cm1, cm2, n == 0);
        if (stats_out != nullptr) {
            float* o = stats_out + (size_t)b * 4;
            o[0] = c0; o[1] = c1; o[2] = c2; o[3] = k;
        }
    }
    // ---- pass 4: apply
    const bool nrm_scale = sp.scale != 0;
    const double is0 = 1.0 / (double)P.sc0, is1 = 1.0 / (double)P.sc1, is2 = 1.0 / (double)P.sc2;
    for (long long trip = 0; trip < trips; ++trip) {
        long long l0;
        const int nv = rows_of(trip, l0);
        if (nv <= 0) continue;                                   // (no barrier below)
        if (!resident) seg_ld12(cpos + 3 * l0, nv, v);
        float nz[12], nm[12];
        if (sp.noise) {
            if (noise_in != nullptr) {
                seg_ld12(noise_in + 3 * (r_lo + l0), nv, nz);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) nz[j] = aug_noise_draw(sp.sigma, seed, ctr, b, AUG_SLOT_NOISE + 3ull * (unsigned long long)l0 + j);
            }
        }
        if (norm != nullptr) seg_ld12(norm + 3 * (r_lo + l0), nv, nm);
#pragma unroll
        for (int j = 0; j < SEG_PPT; ++j) {
            float px = v[3 * j], py = v[3 * j + 1], pz = v[3 * j + 2];
            place(px, py, pz);
            aug_flip_noise(sp, P, cm0, cm1, cm2, nz + 3 * j, px, py, pz);
            v[3 * j] = px; v[3 * j + 1] = py; v[3 * j + 2] = pz;
            if (norm != nullptr) {
                float ax = nm[3 * j], ay = nm[3 * j + 1], az = nm[3 * j + 2];
                aug_rotate_scale(sp.rotate_axis, 0, P, ax, ay, az);
                if (nrm_scale) {                                 // n_i / s_i, then unit length: in double, rounded once per component
                    const double dx = (double)ax * is0, dy = (double)ay * is1, dz = (double)az * is2;
                    const double len = sqrt(dx * dx + dy * dy + dz * dz);
                    if (len > 0.0) {
                        const double il = 1.0 / len;
                        ax = (float)(dx * il); ay = (float)(dy * il); az = (float)(dz * il);
                    } else {
                        ax = (float)dx; ay = (float)dy; az = (float)dz;
                    }
                }
                if (P.flip & 1) ax = -ax;
                if (P.flip & 2) ay = -ay;
                if (P.flip & 4) az = -az;
                nm[3 * j] = ax; nm[3 * j + 1] = ay; nm[3 * j + 2] = az;
            }
        }
        seg_st12(cpos + 3 * l0, nv, v);
        if (norm != nullptr) seg_st12(norm + 3 * (r_lo + l0), nv, nm);
        if (x == nullptr) continue;
        if (C == 3) {
            seg_st12(x + 3 * (r_lo + l0), nv, v);
            continue;
        }
        // C == 6: rows [p0 p1 p2 | n0 n1 n2] or [p0 p1 p2 | rgb]: the rgb half is never read, only zeroed on a drop
        float* xr = x + 6 * (r_lo + l0);
#pragma unroll
        for (int j = 0; j < SEG_PPT; ++j) {
            if (j < nv) {
                xr[6 * j] = v[3 * j]; xr[6 * j + 1] = v[3 * j + 1]; xr[6 * j + 2] = v[3 * j + 2];
                if (sp.x_norm) { xr[6 * j + 3] = nm[3 * j]; xr[6 * j + 4] = nm[3 * j + 1]; xr[6 * j + 5] = nm[3 * j + 2]; }
                else if (!P.keep) { xr[6 * j + 3] = 0.f; xr[6 * j + 4] = 0.f; xr[6 * j + 5] = 0.f; }
            }
        }
    }
}

// ------------------------------------------------------------------ PyG FixedPoints(num, replace, allow_duplicates) per cloud
// Cloud b holds n_b = ptr[b + 1] - ptr[b] rows and receives m_b = out_ptr[b + 1] - out_ptr[b] picks, GLOBAL rows, at
// index[out_ptr[b] ..].  h(b, j) is splitmix64's finisher over (seed ^ FXP_DOMAIN, *counter, b, j); *counter is a device word.
//   mode 0 (replace)            pick t = ((h(b, t) >> 32) * n_b) >> 32, the dilated tables' form (duplicates stay)
//   mode 1 (without replacement) row j has the key h(b, j); the picks are the rows with the min(m_b, n_b) smallest keys, ties to the
//                               lower j, in ASCENDING ROW ORDER; slots beyond n_b hold -1
//   mode 2 (allow_duplicates)   floor(m_b / n_b) whole copies of the cloud in row order, then the subset form for the remainder
// An empty cloud with m_b > 0 writes -1.  The subset: an MSB-first radix SELECT of the r-th smallest key, eight passes of 8 bits
// with a 256-bin histogram in LDS (integer adds: the counts do not depend on their order); the keys are recomputed from the hash,
// never stored.  Then one walk in row order: a row is picked when its key is below the r-th, or equals it and fewer than the
// remaining quota of equal keys precede it; its slot is a ballot prefix inside the wavefront plus the earlier wavefronts' counts.
constexpr unsigned long long FXP_DOMAIN = 0x8CB92BA72F3D8DD7ull;

__device__ __forceinline__ unsigned long long fxp_hash(unsigned long long key, unsigned long long j) {
    unsigned long long z = key + j * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(SEG_NT) void fixed_points_kernel(const long long* __restrict__ ptr, const long long* __restrict__ out_ptr,
                                                             long long N, long long M, int mode, unsigned long long seed,
                                                             const long long* __restrict__ counter, long long* __restrict__ index) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    long long r_lo = ptr[b], r_hi = ptr[b + 1], o_lo = out_ptr[b], o_hi = out_ptr[b + 1];
    r_lo = r_lo < 0 ? 0 : (r_lo > N ? N : r_lo);
    r_hi = r_hi < r_lo ? r_lo : (r_hi > N ? N : r_hi);
    o_lo = o_lo < 0 ? 0 : (o_lo > M ? M : o_lo);                 // the picks' slots, kept inside [0, M] whatever out_ptr holds
    o_hi = o_hi < o_lo ? o_lo : (o_hi > M ? M : o_hi);
    const long long n = r_hi - r_lo, m = o_hi - o_lo;
    long long* const out = index + o_lo;
    if (m == 0) return;
    if (n == 0) {
        for (long long t = tid; t < m; t += SEG_NT) out[t] = -1;
        return;
    }
    const unsigned long long key = (seed ^ FXP_DOMAIN) + 0x9E3779B97F4A7C15ull * ((unsigned long long)counter[0] + 1ull)
                                   + (unsigned long long)b * 0xC2B2AE3D27D4EB4Full;
    if (mode == 0) {
        for (long long t = tid; t < m; t += SEG_NT)
            out[t] = r_lo + (long long)(((fxp_hash(key, (unsigned long long)t) >> 32) * (unsigned long long)n) >> 32);
        return;
    }
    long long whole = 0;                                         // slots taken by whole copies of the cloud
    if (mode == 2) {
        whole = (m / n) * n;
        for (long long t = tid; t < whole; t += SEG_NT) out[t] = r_lo + t % n;
    }
    long long r = m - whole;                                     // the subset's size
    if (r > n) {                                                 // (mode 1 with more slots than rows)
        for (long long t = n + tid; t < r; t += SEG_NT) out[whole + t] = -1;
        r = n;
    }
    if (r == 0) return;
    // ---- the r-th smallest key T (rank r - 1) and how many keys lie below it
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_wsum[SEG_NW];
    __shared__ unsigned long long s_prefix;
    __shared__ long long s_rank;
    unsigned long long prefix = 0;                               // the digits found, high-aligned
    long long rank = r - 1;                                      // rank wanted among the keys that match them
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) s_hist[tid] = 0u;
        __syncthreads();
        for (long long j = tid; j < n; j += SEG_NT) {
            const unsigned long long h = fxp_hash(key, (unsigned long long)j);
            if (pass == 0 || (h >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(unsigned)(h >> shift) & 255u], 1u);
        }
        __syncthreads();
        // inclusive scan of the 256 bins by the first four wavefronts; the bin whose range holds `rank` reports itself
        unsigned cnt = 0u, inc = 0u;
        if (tid < 256) {
            cnt = s_hist[tid];
            inc = cnt;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const unsigned up = __shfl_up(inc, o, WAVE);
                if (lane >= o) inc += up;
            }
            if (lane == WAVE - 1) s_wsum[w] = inc;
        }
        __syncthreads();
        if (tid < 256) {
            unsigned before = 0u;
            for (int q = 0; q < w; ++q) before += s_wsum[q];
            const long long lo = (long long)before + (long long)(inc - cnt), hi = (long long)before + (long long)inc;
            if (rank >= lo && rank < hi) {                       // exactly one bin
                s_prefix = prefix | ((unsigned long long)tid << shift);
                s_rank = rank - lo;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
        __syncthreads();                                         // (s_hist, s_wsum, s_prefix are written again in the next pass)
    }
    const unsigned long long T = prefix;
    const long long need_eq = rank + 1;                          // of the keys equal to T, the first need_eq rows are picked
    // ---- one walk in row order
    __shared__ unsigned s_lt[SEG_NW], s_eq[SEG_NW];
    long long base_lt = 0, base_eq = 0;                          // rows below T / equal to T in the chunks walked so far
    for (long long j0 = 0; j0 < n; j0 += SEG_NT) {
        const long long j = j0 + tid;
        bool lt = false, eq = false;
        if (j < n) {
            const unsigned long long h = fxp_hash(key, (unsigned long long)j);
            lt = h < T;
            eq = h == T;
        }
        const unsigned long long vlt = __ballot(lt), veq = __ballot(eq);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) { s_lt[w] = (unsigned)__popcll(vlt); s_eq[w] = (unsigned)__popcll(veq); }
        __syncthreads();
        long long lt_before = base_lt + __popcll(vlt & below), eq_before = base_eq + __popcll(veq & below), lt_all = 0, eq_all = 0;
#pragma unroll
        for (int q = 0; q < SEG_NW; ++q) {
            if (q < w) { lt_before += s_lt[q]; eq_before += s_eq[q]; }
            lt_all += s_lt[q]; eq_all += s_eq[q];
        }
        if (lt || (eq && eq_before < need_eq)) {
            const long long slot = lt_before + (eq_before < need_eq ? eq_before : need_eq);
            if (slot < r) out[whole + slot] = r_lo + j;          // (always: exactly r rows qualify)
        }
        base_lt += lt_all;
        base_eq += eq_all;
        __syncthreads();
    }
}

}  // namespace crf

using namespace crf;

extern "C" int crfconv_augment_segments(float* pos, float* norm, float* x, int64_t N, int C, const int64_t* ptr, int64_t S,
                                        const crf_augment_segments_spec* spec, uint64_t seed, const int64_t* counter,
                                        const float* params_in, const float* noise_in, float* params_out, float* stats_out,
                                        crf_stream_t stream) {
    CRF_REQUIRE(spec && counter && ptr, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(N >= 0 && N < ((int64_t)1 << 40) && S >= 0 && S <= 0x7fffffff, CRF_ERR_ARG, "bad shape N=%lld S=%lld", (long long)N,
                (long long)S);
    CRF_REQUIRE(pos != nullptr || N == 0, CRF_ERR_ARG, "null pos");
    CRF_REQUIRE(x == nullptr || C == 3 || C == 6, CRF_ERR_ARG, "x has C=%d channels (3 or 6: [pos], [pos, rgb] or [pos, norm])", C);
    const crf_augment_segments_spec sp = *spec;
    CRF_REQUIRE((sp.center == 0 || sp.center == 1) && (sp.normalize == 0 || sp.normalize == 1) && (sp.x_norm == 0 || sp.x_norm == 1),
                CRF_ERR_ARG, "center / normalize / x_norm flags must be 0 or 1");
    CRF_REQUIRE(!sp.x_norm || (x != nullptr && C == 6 && norm != nullptr), CRF_ERR_ARG, "the [pos, norm] layout needs x with C = 6 and norm");
    if (int rc = aug_check_spec(sp)) return rc;
    auto al4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; };
    CRF_REQUIRE(al4(pos) && al4(norm) && al4(x) && al4(noise_in), CRF_ERR_ARG, "arrays must be 4-byte aligned");
    if (S == 0) return CRF_OK;
    hipLaunchKernelGGL(aug_segments_kernel, dim3((unsigned)S), dim3(SEG_NT), 0, as_stream(stream), pos, norm, x, (long long)N, C,
                       reinterpret_cast<const long long*>(ptr), sp, (unsigned long long)seed,
                       reinterpret_cast<const long long*>(counter), params_in, noise_in, params_out, stats_out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_fixed_points(const int64_t* ptr, const int64_t* out_ptr, int64_t S, int64_t N, int64_t M, int mode, uint64_t seed,
                                    const int64_t* counter, int64_t* index, crf_stream_t stream) {
    CRF_REQUIRE(ptr && out_ptr && counter, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(mode >= 0 && mode <= 2, CRF_ERR_ARG, "mode=%d outside {0: replace, 1: without replacement, 2: allow_duplicates}", mode);
    CRF_REQUIRE(N >= 0 && N < ((int64_t)1 << 32) && M >= 0 && S >= 0 && S <= 0x7fffffff, CRF_ERR_ARG, "bad shape S=%lld N=%lld M=%lld",
                (long long)S, (long long)N, (long long)M);
    CRF_REQUIRE(index != nullptr || M == 0, CRF_ERR_ARG, "null index");
    if (S == 0 || M == 0) return CRF_OK;
    hipLaunchKernelGGL(fixed_points_kernel, dim3((unsigned)S), dim3(SEG_NT), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(ptr), reinterpret_cast<const long long*>(out_ptr), (long long)N, (long long)M, mode,
                       (unsigned long long)seed, reinterpret_cast<const long long*>(counter), reinterpret_cast<long long*>(index));
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
