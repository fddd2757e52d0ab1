// What the crop paths of sampler.hip share -- the single-crop entry with its full sort and the batch forms with their select: every
// piece of arithmetic the bit-for-bit guarantees rest on (batch = loop of single crops = the reference's fixtures) is written here
// once.  Workgroups of CROP_NT = 256 threads throughout.
#pragma once
#include "common.hpp"

namespace crf {

constexpr int CROP_NT = 256;

// ---- arg-min with the first index on ties (np.argmin)
struct MinIdx {
    double v;
    long long i;
};
__device__ __forceinline__ MinIdx min_none() { return MinIdx{1.0 / 0.0, INT64_MAX}; }
__device__ __forceinline__ MinIdx min_first(MinIdx a, MinIdx b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ MinIdx wave_min_first(MinIdx m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MinIdx other;
        other.v = __shfl_xor(m.v, o, WAVE);
        other.i = __shfl_xor(m.i, o, WAVE);
        m = min_first(m, other);
    }
    return m;
}
__device__ __forceinline__ MinIdx block_min_first(MinIdx m) {      // the whole workgroup calls; valid on thread 0
    __shared__ double s_v[CROP_NT / WAVE];
    __shared__ long long s_i[CROP_NT / WAVE];
    m = wave_min_first(m);
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = m.v; s_i[threadIdx.x >> 6] = m.i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < CROP_NT / WAVE; ++w) m = min_first(m, MinIdx{s_v[w], s_i[w]});
    return m;
}

// ---- sort key of point i = bit pattern of the float64 squared distance to the seed (sklearn's KDTree holds the points as float64 and
// ranks by the reduced distance sum (x - c)^2); non-negative doubles order like their bit patterns.  x then y then z, every operation
// singly rounded.
__device__ __forceinline__ unsigned long long crop_key(const float* __restrict__ pts, long long i, double cx, double cy, double cz) {
    const double dx = (double)pts[3 * i] - cx, dy = (double)pts[3 * i + 1] - cy, dz = (double)pts[3 * i + 2] - cz;
    const double d = dadd_rn(dadd_rn(dmul_rn(dx, dx), dmul_rn(dy, dy)), dmul_rn(dz, dz));
    return (unsigned long long)__double_as_longlong(d);
}

// ---- float32 distance of point i as the reference forms it for the possibility update
//   Semantic3D (np.sum(np.square(points[q] - pick).astype(np.float32), axis=1), semantic3d_dataset.py:448): squares in float64, each
//   rounded to float32, added left to right in float32;
//   S3DIS (np.sum(np.square(query_xyz.astype(np.float32)), axis=1), s3dis_dataset.py:363): float32 centred coordinates, squares and
//   sums in float32, every operation rounded once.
template <bool S3DIS>
__device__ __forceinline__ float crop_row_dist(const float* __restrict__ points, long long i, const double* __restrict__ center) {
    const double dx = (double)points[3 * i] - center[0], dy = (double)points[3 * i + 1] - center[1], dz = (double)points[3 * i + 2] - center[2];
    if constexpr (S3DIS) {
        const float px = (float)dx, py = (float)dy, pz = (float)dz;
        return add_rn(add_rn(mul_rn(px, px), mul_rn(py, py)), mul_rn(pz, pz));
    } else {
        return add_rn(add_rn((float)dmul_rn(dx, dx), (float)dmul_rn(dy, dy)), (float)dmul_rn(dz, dz));
    }
}

// pmax[blockIdx.x] <- maximum of v over the workgroup (all of its threads call), then d_max over the launch's workgroups
__device__ __forceinline__ void block_max_to(float v, float* __restrict__ pmax) {
    __shared__ float s_red[CROP_NT / WAVE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CROP_NT / WAVE; ++w) v = fmaxf(v, s_red[w]);
        pmax[blockIdx.x] = v;
    }
}
__device__ __forceinline__ float crop_dmax(const float* __restrict__ pmax, int nblk) {
    float dmax = pmax[0];
    for (int b = 1; b < nblk; ++b) dmax = fmaxf(dmax, pmax[b]);
    return dmax;
}

// (1 - d / d_max)^2 in float32, every operation rounded once (no contraction can enter)
__device__ __forceinline__ float crop_gain(float d, float dmax) {
    const float u = sub_rn(1.0f, __fdiv_rn(d, dmax));
    return mul_rn(u, u);
}

// Output row t <- point i: pos centred on the seed in x and y (float64 subtraction rounded to float32; semantic3d_dataset.py:436-437)
// and, with CENTRE_Z, in z as well (s3dis_dataset.py:358); x = [pos] or [pos, rgb], y, point_idx where asked for.
template <bool CENTRE_Z>
__device__ __forceinline__ void crop_write_row(const float* __restrict__ points, const float* __restrict__ rgb,
                                               const int64_t* __restrict__ labels, long long i, const double* __restrict__ center,
                                               long long t, float* __restrict__ out_pos, float* __restrict__ out_x, int xc,
                                               int64_t* __restrict__ out_y, int64_t* __restrict__ out_idx) {
    const float px = (float)((double)points[3 * i + 0] - center[0]);
    const float py = (float)((double)points[3 * i + 1] - center[1]);
    const float pz = CENTRE_Z ? (float)((double)points[3 * i + 2] - center[2]) : points[3 * i + 2];
    out_pos[3 * t + 0] = px;
    out_pos[3 * t + 1] = py;
    out_pos[3 * t + 2] = pz;
    if (out_x != nullptr) {
        float* xr = out_x + (size_t)t * xc;
        xr[0] = px; xr[1] = py; xr[2] = pz;
        if (xc == 6) {
            xr[3] = rgb ? rgb[3 * i + 0] : 0.f;
            xr[4] = rgb ? rgb[3 * i + 1] : 0.f;
            xr[5] = rgb ? rgb[3 * i + 2] : 0.f;
        }
    }
    if (out_y != nullptr) out_y[t] = labels ? labels[i] : 0;
    if (out_idx != nullptr) out_idx[t] = i;
}

// ---- one step of an ORDER-PRESERVING compaction over the workgroup's 256 lanes: compact_count posts how many lanes of this wavefront
// keep their element (s_cnt: CROP_NT / WAVE shared words per predicate), __syncthreads(), then compact_slot gives
// base + (kept lanes before this one) and the workgroup's total; __syncthreads() again before s_cnt is reused.
__device__ __forceinline__ unsigned long long compact_count(bool keep, int* s_cnt) {
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    return m;
}
__device__ __forceinline__ long long compact_slot(unsigned long long m, const int* s_cnt, long long base, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long slot = base + __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < CROP_NT / WAVE; ++w) {
        if (w < wave) slot += s_cnt[w];
        total += s_cnt[w];
    }
    return slot;
}

// ---- a workspace layout stated once: the same pass over take<T>(count) gives the size (base == nullptr) and the pointers.
// Every piece starts on a 256-byte boundary of the (aligned-up) base; bytes() includes the room to align the caller's pointer.
struct Carve {
    char* base;
    size_t off = 0;
    explicit Carve(void* workspace)
        : base(workspace ? reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255) : nullptr) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
    size_t bytes() const { return off + 256; }
};

}  // namespace crf
