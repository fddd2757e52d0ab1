// Per-scene bounds of a ragged batch (pos [N, 3] + ptr [S + 1]) with the check of ptr, and the binary search for a row's scene: what the
// sliding block split (blocks.hip) and the grid subsampling (grid_subsample.hip) share.  The bodies are those blocks.hip held; the bounds
// kernel is a template only because two translation units include this header (as the kernels of radix_sort.hpp and scan.hpp are).
#pragma once
#include "common.hpp"

namespace crf {

enum { SB_BAD_PTR = 1, SB_CELL_CAP = 2, SB_OVERFLOW = 4 };
enum { SB_BLOCKS = 0, SB_ROWS = 1, SB_CELLS = 2, SB_STATUS = 3 };           // totals[]

// order-preserving float <-> uint, branch-free: a negative value has all its bits flipped, any other its sign bit
__device__ __forceinline__ unsigned sb_ord(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float sb_unord(unsigned u) { return __uint_as_float(u ^ (((u >> 31) - 1u) | 0x80000000u)); }

// the scene of row p: the last s with ptr[s] <= p (ptr[0] = 0, ascending; empty scenes repeat an entry and are stepped over)
__device__ __forceinline__ int sb_scene_of(const int64_t* __restrict__ ptr, int S, int64_t p) {
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// bnd [S, 6] uint32: ord(min x, y, z), ord(min -x, -y, -z) -- both sides are atomicMin over a 0xff fill.  A workgroup takes SB_BOUNDS_PPB
// consecutive rows; when they lie in one scene (all but the chunks at scene boundaries) it reduces in registers and every wavefront adds
// six atomics, else every row adds its own.  Also the check of ptr.
constexpr int SB_BOUNDS_PPB = 4096;
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void sb_bounds_kernel(const float* __restrict__ pos, int64_t N, const int64_t* __restrict__ ptr, int S,
                                                        unsigned* __restrict__ bnd, int64_t* __restrict__ totals) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int s = threadIdx.x; s < S; s += 256) {           // every workgroup checks (S is small): a bad ptr stops all of them
        const int64_t lo = ptr[s], hi = ptr[s + 1];
        bad |= lo < 0 || hi < lo || hi > N || (s == 0 && lo != 0) || (s == S - 1 && hi != N);
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) totals[SB_STATUS] = SB_BAD_PTR;
        return;
    }
    const int64_t lo = (int64_t)blockIdx.x * SB_BOUNDS_PPB, hi = lo + SB_BOUNDS_PPB < N ? lo + SB_BOUNDS_PPB : N;
    if (lo >= hi) return;
    const int s_first = sb_scene_of(ptr, S, lo), s_last = sb_scene_of(ptr, S, hi - 1);
    if (s_first == s_last) {
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool any = false;
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
            any = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v = pos[3 * p + a];
                mn[a] = fminf(mn[a], v);
                mx[a] = fmaxf(mx[a], v);
            }
        }
        if (__ballot(any) == 0ull) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            unsigned l = any ? sb_ord(mn[a]) : 0xffffffffu, h = any ? sb_ord(-mx[a]) : 0xffffffffu;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned ol = (unsigned)__shfl_xor((int)l, o, WAVE), oh = (unsigned)__shfl_xor((int)h, o, WAVE);
                l = ol < l ? ol : l;
                h = oh < h ? oh : h;
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&bnd[6 * s_first + a], l);
                atomicMin(&bnd[6 * s_first + 3 + a], h);
            }
        }
    } else {
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
            const int s = sb_scene_of(ptr, S, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v = pos[3 * p + a];
                atomicMin(&bnd[6 * s + a], sb_ord(v));
                atomicMin(&bnd[6 * s + 3 + a], sb_ord(-v));
            }
        }
    }
}

}  // namespace crf
