// Farthest point sampling (torch_cluster.fps as used by the reference's sparse graph builder, models/point_conv.py:381, and
// tpcuda.furthest_point_sampling of the collate, datasets/semantic3d_dataset.py:520).  Inherently sequential in the number of picks:
// pick t + 1 is the point whose distance to picks 0 ... t is largest.  ONE 1024-thread workgroup per cloud, point i held by thread
// i % 1024, and a workgroup waits for nothing outside itself -- a cloud split over CUs would pay a global round trip per pick.
//
// The cloud sizes are device data, so ONE kernel branches per workgroup on its cloud's n (uniform for the workgroup):
//
//   n <= 64              one wavefront, no barrier at all: the other fifteen return before the first pick.
//   n <= 16 384          RESIDENT<R>, R = ceil(n / 1024) = 1 ... 16: x, y, z and the running minimum distance of every point stay in
//                        registers for all picks.  The pick loop stores the pick and touches no other global memory.
//   n <= 65 536          DISTANCES RESIDENT: the minimum distances stay in registers (64 per thread), positions stream from L2
//                        (read-only: no store-then-load chain).
//   larger               STREAMING: the round-1 loop, distances in global memory.
//
// Arg-max: one 64-bit key per thread, high word = the distance's bits (distances are >= +0, so their bits order as unsigned), low word
// = ~index (ties go to the lower index; the key of a thread without a point is 0, below every real key).  Within the wavefront the
// keys are reduced by DPP row shifts and row broadcasts; the lane that holds the wavefront's maximum writes {key, its point's x, y, z}
// into the wavefront's LDS slot; ONE workgroup barrier; then every wavefront reduces the (up to) 16 slot keys for itself and reads
// the winner's coordinates from the winner's slot -- the winner's wavefront is bits 6 ... 9 of its index.  The slots are double-buffered
// on the pick's parity: a wavefront can write pick t + 2 only after the barrier of pick t + 1, which every reader of pick t has reached.
// Wavefronts past the cloud's last point hold no point: they skip the arithmetic and only arrive at the barrier.
//
// ONE distance function for all tiers, in the operation order the round-1 kernel compiled to (dx^2, then fma(dy, dy, .), then + dz^2),
// so that which tier ran never decides a pick and the picks are the earlier kernel's bit for bit.
#include "common.hpp"

namespace crf {

__device__ __forceinline__ float fps_sqdist(float px, float py, float pz, float cx, float cy, float cz) {
    const float dx = sub_rn(px, cx), dy = sub_rn(py, cy), dz = sub_rn(pz, cz);
    return add_rn(__fmaf_rn(dy, dy, mul_rn(dx, dx)), mul_rn(dz, dz));
}

constexpr float FPS_FAR = 3.4e38f;        // a point's distance before the first pick
constexpr int FPS_NT = 1024, FPS_WAVES = FPS_NT / WAVE;

__device__ __forceinline__ unsigned long long fps_key(float best, int index) {
    return best < 0.f ? 0ull : ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)~(unsigned)index;
}

// max(k, the key of the lane that the DPP control names); a lane without a source, or in a row outside ROW_MASK, keeps its own
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long key_max_dpp(unsigned long long k) {
    const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o > k ? o : k;
}
__device__ __forceinline__ unsigned long long key_of_lane(unsigned long long k, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
// lane 15 of every row of 16 lanes ends with the row's maximum: row_shr 1, 2, 4, 8
__device__ __forceinline__ unsigned long long row_key_max(unsigned long long k) {
    k = key_max_dpp<0x111, 0xf>(k);
    k = key_max_dpp<0x112, 0xf>(k);
    k = key_max_dpp<0x114, 0xf>(k);
    return key_max_dpp<0x118, 0xf>(k);
}
// the wavefront's maximum, uniform: rows, then row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3, lane 63 has it
__device__ __forceinline__ unsigned long long wave_key_max(unsigned long long k) {
    k = row_key_max(k);
    k = key_max_dpp<0x142, 0xa>(k);
    k = key_max_dpp<0x143, 0xc>(k);
    return key_of_lane(k, 63);
}

struct FpsShared {
    unsigned long long key[2][FPS_WAVES];      // [pick parity][wavefront]
    float4 xyz[2][FPS_WAVES];
    float4 start;                               // the first pick's coordinates
    float sval[FPS_WAVES];                      // streaming tier
    int sidx[FPS_WAVES];
    int scur;
};

// The workgroup's maximum of the slot keys of pick parity `par`, uniform (every wavefront for itself).
__device__ __forceinline__ unsigned long long slots_key_max(const FpsShared& sh, int par, int nwa) {
    const int slot = threadIdx.x & 15;
    return key_of_lane(row_key_max(slot < nwa ? sh.key[par][slot] : 0ull), 15);
}

// n <= 64: wavefront 0 alone (the caller returned the others), lane i holds point i.
__device__ __forceinline__ void fps_one_wave(const float* __restrict__ p, int n, int m, int cur, int64_t s0, int64_t* __restrict__ o) {
    const int lane = threadIdx.x;
    const bool has = lane < n;
    const float x = has ? p[3 * lane] : 0.f, y = has ? p[3 * lane + 1] : 0.f, z = has ? p[3 * lane + 2] : 0.f;
    float d = has ? FPS_FAR : -1.f;
    for (int t = 0;; ++t) {
        if (lane == 0) o[t] = s0 + cur;
        if (t + 1 >= m) break;
        const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), cur)), cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), cur)),
                    cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), cur));
        d = fminf(d, fps_sqdist(x, y, z, cx, cy, cz));
        cur = (int)~(unsigned)wave_key_max(fps_key(d, lane));
    }
}

template <int R>
__device__ __forceinline__ void fps_resident(const float* __restrict__ p, int n, int m, int first, int64_t s0, int64_t* __restrict__ o, FpsShared& sh) {
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nwa = n >= FPS_NT ? FPS_WAVES : (n + WAVE - 1) / WAVE;       // wavefronts that hold a point
    const bool active = wave < nwa;
    float x[R], y[R], z[R], d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + FPS_NT * r;
        const bool has = i < n;
        x[r] = has ? p[3 * i] : 0.f;
        y[r] = has ? p[3 * i + 1] : 0.f;
        z[r] = has ? p[3 * i + 2] : 0.f;
        d[r] = has ? FPS_FAR : -1.f;                                        // -1: never above `best`, whatever the pick
    }
    if (tid == (first & (FPS_NT - 1))) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == (first >> 10)) c = make_float4(x[r], y[r], z[r], 0.f);
        sh.start = c;
    }
    __syncthreads();
    int cur = first;
    float cx = sh.start.x, cy = sh.start.y, cz = sh.start.z;
    for (int t = 0;; ++t) {
        if (tid == 0) o[t] = s0 + cur;
        if (t + 1 >= m) break;
        const int par = t & 1;
        if (active) {
            float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
            int br = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float dd = fminf(d[r], fps_sqdist(x[r], y[r], z[r], cx, cy, cz));
                d[r] = dd;
                if (dd > best) { best = dd; br = r; bx = x[r]; by = y[r]; bz = z[r]; }
            }
            const unsigned long long key = fps_key(best, tid + FPS_NT * br);
            if (key == wave_key_max(key)) {                                 // one lane: an active wavefront holds a point, and keys of points are distinct
                sh.key[par][wave] = key;
                sh.xyz[par][wave] = make_float4(bx, by, bz, 0.f);
            }
        }
        __syncthreads();
        if (active) {
            cur = (int)~(unsigned)slots_key_max(sh, par, nwa);
            const float4 c = sh.xyz[par][(cur >> 6) & (FPS_WAVES - 1)];
            cx = c.x; cy = c.y; cz = c.z;
        }
    }
}

// 16 384 < n <= 65 536: every wavefront holds points.  Rows of 1024 points go in chunks of eight, whose loads are in flight together; a
// chunk past the cloud is skipped (uniform), a row past the cloud's end loads the thread's first point instead.
constexpr int FPS_DR = 64, FPS_CHUNK = 8;
__device__ __forceinline__ void fps_dist_resident(const float* __restrict__ p, int n, int m, int first, int64_t s0, int64_t* __restrict__ o, FpsShared& sh) {
    const int tid0 = threadIdx.x, wave = tid0 >> 6;
    float d[FPS_DR];
#pragma unroll
    for (int r = 0; r < FPS_DR; ++r) d[r] = tid0 + FPS_NT * r < n ? FPS_FAR : -1.f;
    int cur = first;
    for (int t = 0;; ++t) {
        if (tid0 == 0) o[t] = s0 + cur;
        if (t + 1 >= m) break;
        const int par = t & 1;
        const float cx = p[3 * cur], cy = p[3 * cur + 1], cz = p[3 * cur + 2];
        float best = -1.f;
        int bi = 0, tid = tid0;
        asm volatile("" : "+v"(tid));        // (addresses re-derived per pick: 128 hoisted 64-bit row addresses would be kept alive -- and spilled)
        static_for<FPS_DR / FPS_CHUNK>([&](auto chunk) {
            constexpr int r0 = decltype(chunk)::value * FPS_CHUNK;
            if (FPS_NT * r0 >= n) return;
            float px[FPS_CHUNK], py[FPS_CHUNK], pz[FPS_CHUNK];
#pragma unroll
            for (int k = 0; k < FPS_CHUNK; ++k) {                            // the chunk's loads, all in flight together
                const int i = tid + FPS_NT * (r0 + k);
                const float* q = p + 3 * (int64_t)(i < n ? i : tid);         // (a row past the end: d = -1 keeps it out)
                px[k] = q[0]; py[k] = q[1]; pz[k] = q[2];
            }
#pragma unroll
            for (int k = 0; k < FPS_CHUNK; ++k) {
                const float dd = fminf(d[r0 + k], fps_sqdist(px[k], py[k], pz[k], cx, cy, cz));
                d[r0 + k] = dd;
                if (dd > best) { best = dd; bi = tid + FPS_NT * (r0 + k); }
            }
        });
        const unsigned long long key = fps_key(best, bi);
        if (key == wave_key_max(key)) sh.key[par][wave] = key;
        __syncthreads();
        cur = (int)~(unsigned)slots_key_max(sh, par, FPS_WAVES);
    }
}

// n > 65 536: the running minimum distances in global memory (L2-resident), min-update + arg-max per pick.
__device__ __forceinline__ void fps_streaming(const float* __restrict__ p, int64_t n, int64_t m, int first, int64_t s0, float* __restrict__ d,
                                              int64_t* __restrict__ o, FpsShared& sh) {
    for (int64_t i = threadIdx.x; i < n; i += FPS_NT) d[i] = FPS_FAR;
    if (threadIdx.x == 0) sh.scur = first;
    __syncthreads();
    for (int64_t t = 0; t < m; ++t) {
        const int cur = sh.scur;
        if (threadIdx.x == 0) o[t] = s0 + cur;
        const float cx = p[3 * cur], cy = p[3 * cur + 1], cz = p[3 * cur + 2];
        float best = -1.f;
        int bi = 0x7fffffff;
        for (int64_t i = threadIdx.x; i < n; i += FPS_NT) {
            const float dd = fminf(d[i], fps_sqdist(p[3 * i], p[3 * i + 1], p[3 * i + 2], cx, cy, cz));
            d[i] = dd;
            if (dd > best) { best = dd; bi = (int)i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, WAVE);
            const int oi = __shfl_xor(bi, off, WAVE);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();                                   // scur consumed by everyone
        if (lane == 0) { sh.sval[wave] = best; sh.sidx[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float bv = sh.sval[0];
            int bj = sh.sidx[0];
            for (int w = 1; w < FPS_WAVES; ++w)
                if (sh.sval[w] > bv || (sh.sval[w] == bv && sh.sidx[w] < bj)) { bv = sh.sval[w]; bj = sh.sidx[w]; }
            sh.scur = bj;
        }
        __syncthreads();
    }
}

// f(std::integral_constant<int, R>{}) for the R of the list that equals r (uniform): common.hpp's dispatch_width, on the device
template <int... Rs, class F>
__device__ __forceinline__ void rows_dispatch(Widths<Rs...>, int r, F&& f) {
    (void)((r == Rs && (f(std::integral_constant<int, Rs>{}), true)) || ...);
}

constexpr int FPS_RESIDENT_MAX = 16 * FPS_NT, FPS_DIST_RESIDENT_MAX = FPS_DR * FPS_NT;

// Everything the branches below look at is uniform for the workgroup: the pick count m is read once and clamped to [0, n], the first
// pick to [0, n); an empty cloud or no pick is a clean return.
__global__ __launch_bounds__(FPS_NT) void fps_kernel(const float* __restrict__ pos, const int64_t* __restrict__ seg_start,
                                                     const int64_t* __restrict__ seg_count, const int64_t* __restrict__ out_start,
                                                     const int64_t* __restrict__ n_sample, const int64_t* __restrict__ first,
                                                     float* __restrict__ dist, int64_t* __restrict__ out) {
    const int c = blockIdx.x;
    const int64_t s0 = uni((long long)seg_start[c]), n = uni((long long)seg_count[c]);
    int64_t m = uni((long long)n_sample[c]), f = uni((long long)first[c]);
    if (n <= 0 || m <= 0) return;
    m = m < n ? m : n;
    f = f < 0 ? 0 : (f < n ? f : n - 1);
    const float* p = pos + 3 * s0;
    int64_t* o = out + uni((long long)out_start[c]);
    __shared__ FpsShared sh;
    if (n <= WAVE) {
        if (threadIdx.x < WAVE) fps_one_wave(p, (int)n, (int)m, (int)f, s0, o);
    } else if (n <= FPS_RESIDENT_MAX) {
        rows_dispatch(Widths<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>{}, (int)((n + FPS_NT - 1) / FPS_NT),
                      [&](auto R) { fps_resident<decltype(R)::value>(p, (int)n, (int)m, (int)f, s0, o, sh); });
    } else if (n <= FPS_DIST_RESIDENT_MAX) {
        fps_dist_resident(p, (int)n, (int)m, (int)f, s0, o, sh);
    } else {
        fps_streaming(p, n, m, (int)f, s0, dist + s0, o, sh);
    }
}

#ifdef CRF_FPS_PROBE
// One kernel per form, for the resource table of profiles/ (scratch/fps_resources.sh compiles the unit with -DCRF_FPS_PROBE).
template <int R>
__global__ __launch_bounds__(FPS_NT) void fps_probe_resident(const float* p, int n, int m, int first, int64_t* o) {
    __shared__ FpsShared sh;
    fps_resident<R>(p, n, m, first, 0, o, sh);
}
#define CRF_FPS_PROBE_R(R) template __global__ void fps_probe_resident<R>(const float*, int, int, int, int64_t*);
CRF_FPS_PROBE_R(1) CRF_FPS_PROBE_R(2) CRF_FPS_PROBE_R(3) CRF_FPS_PROBE_R(4) CRF_FPS_PROBE_R(5) CRF_FPS_PROBE_R(6) CRF_FPS_PROBE_R(7) CRF_FPS_PROBE_R(8)
CRF_FPS_PROBE_R(9) CRF_FPS_PROBE_R(10) CRF_FPS_PROBE_R(11) CRF_FPS_PROBE_R(12) CRF_FPS_PROBE_R(13) CRF_FPS_PROBE_R(14) CRF_FPS_PROBE_R(15) CRF_FPS_PROBE_R(16)
__global__ __launch_bounds__(FPS_NT) void fps_probe_dist_resident(const float* p, int n, int m, int first, int64_t* o) {
    __shared__ FpsShared sh;
    fps_dist_resident(p, n, m, first, 0, o, sh);
}
__global__ __launch_bounds__(FPS_NT) void fps_probe_streaming(const float* p, int64_t n, int64_t m, int first, float* d, int64_t* o) {
    __shared__ FpsShared sh;
    fps_streaming(p, n, m, first, 0, d, o, sh);
}
__global__ __launch_bounds__(WAVE) void fps_probe_one_wave(const float* p, int n, int m, int first, int64_t* o) { fps_one_wave(p, n, m, first, 0, o); }
#endif

}  // namespace crf

extern "C" int crfconv_fps(const float* pos, int n_clouds, const int64_t* seg_start, const int64_t* seg_count,
                           const int64_t* out_start, const int64_t* n_sample, const int64_t* first, float* dist_ws,
                           int64_t* out, crf_stream_t stream) {
    CRF_REQUIRE(pos && seg_start && seg_count && out_start && n_sample && first && dist_ws && out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(n_clouds >= 1 && n_clouds <= 65535, CRF_ERR_ARG, "n_clouds=%d out of range", n_clouds);
    hipLaunchKernelGGL(crf::fps_kernel, dim3(n_clouds), dim3(crf::FPS_NT), 0, crf::as_stream(stream), pos, seg_start, seg_count,
                       out_start, n_sample, first, dist_ws, out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
