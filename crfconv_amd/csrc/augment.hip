// The reference's training augmentation (trainval.py:26-36: RandomRotate -> RandomScaleAnisotropic -> RandomSymmetry -> RandomNoise
// -> DropFeature -> AddFeatsByKeys) on a batch of crops pos [B, N, 3] (+ x [B, N, C], C in {3, 6}, layout [pos, rgb]), in place,
// ahead of the collate's Morton sort and neighbour tables (crfconv_amd.transforms.Compose; data.CollateGraph(augment=) runs it
// inside the captured collate graph).
//
//   per cloud   cos / sin of theta ~ U(deg_lo, deg_hi) degrees about `axis`, three scales ~ U(s_lo, s_lo + s_span), a flip bit per
//               axis (probability 1/2), a keep bit (the crop's rgb survives with probability 1 - p).  Every parameter is a 24-bit
//               uniform (exact in fp32) of a splitmix64 hash of (seed ^ AUG_DOMAIN, *counter, cloud, slot) -- *counter is a DEVICE
//               word, so a captured graph draws new parameters at every replay.  Host twin: transforms.Compose.draws.
//   per point   pos <- rot.scale(pos); flipped axis i: pos_i <- c_max_i - pos_i (c_max_i = the cloud's max of rot.scale pos_i);
//               pos += clamp(sigma N(0, 1), -clip, clip) (Box-Muller of two 24-bit uniforms of a hash of (cloud, point, axis));
//               x[..., 0:3] <- pos, x[..., 3:6] <- 0 when the keep bit is 0.
//
// Launches: one (aug_apply_kernel) -- or two when an axis may flip: aug_max_kernel writes one partial max per workgroup and axis
// into the workspace, and every workgroup of aug_apply_kernel reduces its own cloud's partials (no atomics, nothing to zero,
// bitwise deterministic, capturable).  Both go through aug_rotate_scale, singly rounded operations (no FMA contraction): a flipped
// cloud's minimum is then exactly 0 without noise.  A lane owns four consecutive points: 3 x 16-byte loads of pos (6 of x at C = 6)
// when the rows are 16-byte aligned (N % 4 == 0), per-point dwords otherwise.
#include "augment_common.hpp"

namespace crf {

constexpr int AUG_NT = 256, AUG_PPT = 4, AUG_PPB = AUG_NT * AUG_PPT;

// the lane's points [4 g, 4 g + 4) of cloud b (n of them valid): 12 floats of a [.., 3] row block, vector loads when aligned
__device__ __forceinline__ void aug_load3(const float* __restrict__ base, int n, bool vec, float (&v)[12]) {
    if (vec && n == AUG_PPT) {
        const float4 a = ld4(base), b = ld4(base + 4), c = ld4(base + 8);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * n) v[j] = base[j];
    }
}

// max over the workgroup of v (every lane contributes; -inf = nothing); the result is valid in thread 0
__device__ __forceinline__ float aug_block_max(float v, float* s_red) {
    v = group_max<WAVE>(v);
    const int w = threadIdx.x / WAVE;
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < AUG_NT / WAVE; ++k) v = fmaxf(v, s_red[k]);
    }
    return v;
}

// workspace [B, nblk, 4]: the workgroup's max of rot.scale pos per axis (slot 3 unused)
__global__ __launch_bounds__(AUG_NT) void aug_max_kernel(const float* __restrict__ pos, int N, bool vec, const crf_augment_spec sp,
                                                        unsigned long long seed, const long long* __restrict__ counter,
                                                        const float* __restrict__ params_in, float* __restrict__ partial) {
    const int b = blockIdx.y;
    const unsigned long long ctr = (unsigned long long)counter[0];
    const AugParams P = aug_cloud_params(sp, seed, ctr, b, params_in);
    const int g = blockIdx.x * AUG_NT + threadIdx.x;
    const int i0 = g * AUG_PPT, n = N - i0 < 0 ? 0 : (N - i0 < AUG_PPT ? N - i0 : AUG_PPT);
    float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY;
    if (n > 0) {
        float v[12];
        aug_load3(pos + ((size_t)b * N + i0) * 3, n, vec, v);
#pragma unroll
        for (int j = 0; j < AUG_PPT; ++j) {
            float x = v[3 * j], y = v[3 * j + 1], z = v[3 * j + 2];
            aug_rotate_scale(sp, P, x, y, z);
            if (j < n) { m0 = fmaxf(m0, x); m1 = fmaxf(m1, y); m2 = fmaxf(m2, z); }
        }
    }
    __shared__ float s_red[AUG_NT / WAVE];
    m0 = aug_block_max(m0, s_red);
    m1 = aug_block_max(m1, s_red);
    m2 = aug_block_max(m2, s_red);
    if (threadIdx.x == 0) {
        float* o = partial + ((size_t)b * gridDim.x + blockIdx.x) * 4;
        o[0] = m0; o[1] = m1; o[2] = m2; o[3] = 0.f;
    }
}

__global__ __launch_bounds__(AUG_NT) void aug_apply_kernel(float* __restrict__ pos, float* __restrict__ x, int N, int C, bool vec,
                                                          const crf_augment_spec sp, unsigned long long seed,
                                                          const long long* __restrict__ counter, const float* __restrict__ params_in,
                                                          const float* __restrict__ noise_in, const float* __restrict__ partial,
                                                          float* __restrict__ params_out) {
    const int b = blockIdx.y;
    // the lane's rows are loaded FIRST: their latency overlaps the counter read, the parameter draws and the partials' reduction
    const int g = blockIdx.x * AUG_NT + threadIdx.x;
    const int i0 = g * AUG_PPT, n = N - i0 < 0 ? 0 : (N - i0 < AUG_PPT ? N - i0 : AUG_PPT);
    float* prow = pos + ((size_t)b * N + i0) * 3;
    float* xrow = x == nullptr ? nullptr : x + ((size_t)b * N + i0) * C;
    const bool full = vec && n == AUG_PPT;
    float v[12], nz[12], r[24];
    if (n > 0) {
        aug_load3(prow, n, vec, v);
        if (sp.noise && noise_in != nullptr) aug_load3(noise_in + ((size_t)b * N + i0) * 3, n, vec, nz);
        if (xrow != nullptr && C == 6 && full) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float4 w = ld4(xrow + 4 * q);
                r[4 * q] = w.x; r[4 * q + 1] = w.y; r[4 * q + 2] = w.z; r[4 * q + 3] = w.w;
            }
        }
    }
    const unsigned long long ctr = (unsigned long long)counter[0];
    const AugParams P = aug_cloud_params(sp, seed, ctr, b, params_in);
    __shared__ float s_red[AUG_NT / WAVE];
    __shared__ float s_cmax[3];
    if (sp.flip_axes != 0) {                         // the cloud's max per axis from the max launch's partials (uniform branch)
        float m[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = threadIdx.x; k < (int)gridDim.x; k += AUG_NT) {
            const float4 q = ld4(partial + ((size_t)b * gridDim.x + k) * 4);
            m[0] = fmaxf(m[0], q.x); m[1] = fmaxf(m[1], q.y); m[2] = fmaxf(m[2], q.z);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float r = aug_block_max(m[i], s_red);
            if (threadIdx.x == 0) s_cmax[i] = r;
        }
        __syncthreads();
    }
    const float cm0 = sp.flip_axes != 0 ? s_cmax[0] : 0.f, cm1 = sp.flip_axes != 0 ? s_cmax[1] : 0.f,
                cm2 = sp.flip_axes != 0 ? s_cmax[2] : 0.f;
    if (params_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
        aug_write_params(params_out + (size_t)b * 8, P, cm0, cm1, cm2, false);
    if (n <= 0) return;
    if (sp.noise) {
        if (noise_in == nullptr) {
#pragma unroll
            for (int k = 0; k < 12; ++k)             // Box-Muller of (cloud, point, axis): augment_common.hpp
                nz[k] = aug_noise_draw(sp.sigma, seed, ctr, b, AUG_SLOT_NOISE + 3ull * (unsigned long long)i0 + k);
        }
    }
#pragma unroll
    for (int j = 0; j < AUG_PPT; ++j) {
        float px = v[3 * j], py = v[3 * j + 1], pz = v[3 * j + 2];
        aug_rotate_scale(sp, P, px, py, pz);
        aug_flip_noise(sp, P, cm0, cm1, cm2, nz + 3 * j, px, py, pz);
        v[3 * j] = px; v[3 * j + 1] = py; v[3 * j + 2] = pz;
    }
    if (full) {
        st4(prow, make_float4(v[0], v[1], v[2], v[3]));
        st4(prow + 4, make_float4(v[4], v[5], v[6], v[7]));
        st4(prow + 8, make_float4(v[8], v[9], v[10], v[11]));
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) prow[k] = v[k];
    }
    if (xrow == nullptr) return;
    if (C == 3) {
        if (full) {
            st4(xrow, make_float4(v[0], v[1], v[2], v[3]));
            st4(xrow + 4, make_float4(v[4], v[5], v[6], v[7]));
            st4(xrow + 8, make_float4(v[8], v[9], v[10], v[11]));
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < 3 * n) xrow[k] = v[k];
        }
        return;
    }
    // C == 6: rows [p0 p1 p2 r0 r1 r2]; the rgb half (loaded above) is kept or zeroed
    if (full) {
#pragma unroll
        for (int j = 0; j < AUG_PPT; ++j) {
            r[6 * j] = v[3 * j]; r[6 * j + 1] = v[3 * j + 1]; r[6 * j + 2] = v[3 * j + 2];
            if (!P.keep) { r[6 * j + 3] = 0.f; r[6 * j + 4] = 0.f; r[6 * j + 5] = 0.f; }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) st4(xrow + 4 * q, make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]));
    } else {
#pragma unroll
        for (int j = 0; j < AUG_PPT; ++j) {
            if (j < n) {
                xrow[6 * j] = v[3 * j]; xrow[6 * j + 1] = v[3 * j + 1]; xrow[6 * j + 2] = v[3 * j + 2];
                if (!P.keep) { xrow[6 * j + 3] = 0.f; xrow[6 * j + 4] = 0.f; xrow[6 * j + 5] = 0.f; }
            }
        }
    }
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_augment_workspace(int64_t B, int64_t N) {
    if (B < 1 || N < 1) return 0;
    return sizeof(float) * 4 * (size_t)(B * cdiv(N, AUG_PPB));
}

extern "C" int crfconv_augment(float* pos, float* x, int64_t B, int64_t N, int C, const crf_augment_spec* spec, uint64_t seed,
                               const int64_t* counter, const float* params_in, const float* noise_in, float* params_out,
                               void* workspace, size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(pos && spec && counter, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N * 6 < ((int64_t)1 << 31), CRF_ERR_ARG, "bad shape B=%lld N=%lld",
                (long long)B, (long long)N);
    CRF_REQUIRE(x == nullptr || C == 3 || C == 6, CRF_ERR_ARG, "x has C=%d channels (3 or 6: [pos] or [pos, rgb])", C);
    const crf_augment_spec sp = *spec;
    if (int rc = aug_check_spec(sp)) return rc;
    const int64_t nblk = cdiv(N, AUG_PPB);
    if (sp.flip_axes != 0)
        CRF_REQUIRE(workspace && workspace_bytes >= crfconv_augment_workspace(B, N) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                    CRF_ERR_WORKSPACE, "workspace too small or misaligned");
    auto al16 = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = N % 4 == 0 && al16(pos) && al16(x) && al16(noise_in);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    const long long* ctr = reinterpret_cast<const long long*>(counter);
    float* partial = static_cast<float*>(workspace);
    if (sp.flip_axes != 0) {
        hipLaunchKernelGGL(aug_max_kernel, grid, dim3(AUG_NT), 0, st, pos, (int)N, vec, sp, (unsigned long long)seed, ctr, params_in, partial);
        CRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(aug_apply_kernel, grid, dim3(AUG_NT), 0, st, pos, x, (int)N, C, vec, sp, (unsigned long long)seed, ctr, params_in,
                       noise_in, sp.flip_axes != 0 ? partial : nullptr, params_out);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
