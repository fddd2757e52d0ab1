// The small dense matrices of the CRF layers: Q = (I + c^T c)^-1 and P = I - Q with their backward (one layer or all layers of a
// network per launch; device bodies in crf_matrices_body.hpp, which the launches that carry them as riders share), and the two
// SPD inverses spd_inverse_kernel (H <= 64, registers) and spd_inverse_wide_kernel (H <= 512, the sparse networks).
#include "common.hpp"
#include "crf_matrices_body.hpp"

namespace crf {

// ------------------------------------------------------------------ (I + C)^-1 for the CRF layers
// In-place Gauss-Jordan on the H x H (H <= 64) symmetric positive definite matrix M = I + c^T c
// (models/continuous_crf_conv_big.py:72 calls .inverse() inside the loop; it is loop invariant).  No pivoting
// needed (eigenvalues >= 1), float64 throughout.  One workgroup of 16 x 16 threads; thread (tr, tc) keeps the 4 x 4
// cyclic sub-tile rows tr + 16 i, columns tc + 16 j in REGISTERS for the whole elimination, and only the old pivot
// row / column travel through (double-buffered) LDS: one barrier and 16 fused multiply-adds per thread per pivot,
// ~0.1 us a pivot instead of the ~3 us of an all-in-LDS sweep.  Replaces torch.linalg.inv, whose rocSOLVER path
// synchronises and therefore cannot be captured into a hipGraph.
// In-place inverse of the 64 x 64 register-tiled matrix (rows / columns >= H must be identity).
__device__ __forceinline__ void gauss_jordan_tiles(double (&t)[4][4], int H, double (*s_row)[64], double (*s_col)[64]) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {                     // pivot p = 16 ip + pp lives in local row / column ip
        for (int pp = 0; pp < 16; ++pp) {
            const int p = 16 * ip + pp;
            if (p >= H) break;                           // uniform: rows beyond H are identity already
            const int b = p & 1;
            if (tr == pp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s_row[b][tc + 16 * j] = t[ip][j];
            }
            if (tc == pp) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s_col[b][tr + 16 * i] = t[i][ip];
            }
            __syncthreads();
            const double piv = 1.0 / s_row[b][p];
            double rowv[4], colv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) rowv[j] = s_row[b][tc + 16 * j] * piv;
#pragma unroll
            for (int i = 0; i < 4; ++i) colv[i] = s_col[b][tr + 16 * i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool rp = (i == ip) && (tr == pp), cp = (j == ip) && (tc == pp);
                    const double upd = t[i][j] - colv[i] * rowv[j];
                    t[i][j] = rp ? (cp ? piv : rowv[j]) : (cp ? -colv[i] * piv : upd);
                }
        }
    }
}

__global__ __launch_bounds__(256) void spd_inverse_kernel(const float* __restrict__ Min, int H,
                                                          float* __restrict__ Qout) {
    __shared__ double s_row[2][64], s_col[2][64];
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    double t[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tr + 16 * i, c = tc + 16 * j;
            t[i][j] = (r < H && c < H) ? (double)Min[r * H + c] : (r == c ? 1.0 : 0.0);
        }
    gauss_jordan_tiles(t, H, s_row, s_col);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tr + 16 * i, c = tc + 16 * j;
            if (r < H && c < H) Qout[r * H + c] = (float)t[i][j];
        }
}

// All CRF layers of a network in ONE launch (one workgroup each; CrfMatJobs: crf_matrices_body.hpp)
__global__ __launch_bounds__(CMF_BLOCK) void crf_matrices_batched_kernel(const CrfMatJobs j) {
    const int b = blockIdx.x;
    __shared__ __attribute__((aligned(16))) char lds[CMF_LDS_BYTES];
    crf_matrices_body(j.c[b], j.H[b], j.Q[b], j.P[b], lds);
}

__global__ __launch_bounds__(CMB_BLOCK) void crf_matrices_bwd_kernel(const float* __restrict__ cmat, const float* __restrict__ Q,
                                                               const float* __restrict__ dQ, const float* __restrict__ dP,
                                                               int H, float* __restrict__ dc) {
    crf_matrices_bwd_slab(cmat, Q, dQ, dP, H, (int)blockIdx.x * CMB_ROWS, dc);
}
__global__ __launch_bounds__(CMB_BLOCK) void crf_matrices_bwd_batched_kernel(const CrfMatJobs j) {
    int b = 0;                                                  // layer of this workgroup: slab_base is a prefix over the layers
    while (b + 1 < CM_MAX && (int)blockIdx.x >= j.slab_base[b + 1]) ++b;
    crf_matrices_bwd_slab(j.c[b], j.Q_in[b], j.gQ[b], j.gP[b], j.H[b], ((int)blockIdx.x - j.slab_base[b]) * CMB_ROWS, j.dc[b]);
}
}  // namespace crf

extern "C" int crfconv_crf_matrices_batched(const float* const* c, const int* H, int n, float* const* Q, float* const* P,
                                            crf_stream_t stream) {
    CRF_REQUIRE(c && H && Q && P && n >= 1 && n <= crf::CM_MAX, CRF_ERR_ARG, "null pointer or n=%d outside [1, %d]", n, crf::CM_MAX);
    crf::CrfMatJobs j = {};
    for (int i = 0; i < n; ++i) {
        CRF_REQUIRE(c[i] && Q[i] && P[i] && H[i] >= 1 && H[i] <= 64, CRF_ERR_ARG, "job %d: null pointer or H=%d outside [1, 64]", i, H[i]);
        j.c[i] = c[i]; j.Q[i] = Q[i]; j.P[i] = P[i]; j.H[i] = H[i];
    }
    hipLaunchKernelGGL(crf::crf_matrices_batched_kernel, dim3((unsigned)n), dim3(crf::CMF_BLOCK), 0, crf::as_stream(stream), j);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_crf_matrices_backward_batched(const float* const* c, const float* const* Q, const float* const* gQ,
                                                     const float* const* gP, const int* H, int n, float* const* dc,
                                                     crf_stream_t stream) {
    crf::CrfMatJobs j;
    int nslab = 0;
    if (int rc = crf_matrices_bwd_jobs(c, Q, gQ, gP, H, n, dc, j, nslab)) return rc;
    hipLaunchKernelGGL(crf::crf_matrices_bwd_batched_kernel, dim3((unsigned)nslab), dim3(crf::CMB_BLOCK), 0, crf::as_stream(stream), j);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

namespace crf {
// Q = M^-1 for a symmetric positive definite M [H, H] with 64 < H <= 512 (the 128- / 256-channel CRF stages of the sparse networks,
// models/point_conv.py:318-339: M = I + c^T c, eigenvalues >= 1): in-place Gauss-Jordan WITHOUT pivoting on the copy in Q, one
// workgroup, the matrix in global memory behind this CU's caches (256 KB at H = 256 -- it does not fit LDS), pivot row and column
// staged in LDS per step.  H steps of one read-modify-write pass each: ~0.1 ms at H = 128, ~1 ms at H = 256 -- once per forward of
// a layer whose reference recomputes torch.inverse in every mean-field step (continuous_crf_conv.py:66).
constexpr int SW_BLOCK = 1024, SW_MAXH = 512;
__global__ __launch_bounds__(SW_BLOCK) void spd_inverse_wide_kernel(const float* __restrict__ M, int H, float* __restrict__ Q) {
    __shared__ float s_row[SW_MAXH], s_col[SW_MAXH];
    const int n = H * H;
    for (int e = threadIdx.x; e < n; e += SW_BLOCK) Q[e] = M[e];
    __syncthreads();
    for (int k = 0; k < H; ++k) {
        for (int t = threadIdx.x; t < H; t += SW_BLOCK) {
            s_row[t] = Q[k * H + t];
            s_col[t] = Q[t * H + k];
        }
        __syncthreads();
        const float inv = 1.0f / s_row[k];
        for (int e = threadIdx.x; e < n; e += SW_BLOCK) {
            const int i = e / H, j = e - i * H;
            float v;
            if (i == k) v = j == k ? inv : s_row[j] * inv;
            else if (j == k) v = -s_col[i] * inv;
            else v = fmaf(-s_col[i] * inv, s_row[j], Q[e]);
            Q[e] = v;
        }
        __syncthreads();
    }
}
}  // namespace crf

extern "C" int crfconv_spd_inverse_wide(const float* M, int H, float* Q, crf_stream_t stream) {
    CRF_REQUIRE(M && Q && M != Q, CRF_ERR_ARG, "null pointer / aliased operands");
    CRF_REQUIRE(H >= 1 && H <= crf::SW_MAXH, CRF_ERR_UNSUPPORTED, "H=%d outside [1, %d]", H, crf::SW_MAXH);
    hipLaunchKernelGGL(crf::spd_inverse_wide_kernel, dim3(1), dim3(crf::SW_BLOCK), 0, crf::as_stream(stream), M, H, Q);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_spd_inverse(const float* M, int H, float* Q, crf_stream_t stream) {
    CRF_REQUIRE(M && Q, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(H >= 1 && H <= 64, CRF_ERR_UNSUPPORTED, "H=%d outside [1, 64]", H);
    hipLaunchKernelGGL(crf::spd_inverse_kernel, dim3(1), dim3(256), 0, crf::as_stream(stream), M, H, Q);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_crf_matrices_backward(const float* c, const float* Q, const float* dQ, const float* dP, int H,
                                             float* dc, crf_stream_t stream) {
    CRF_REQUIRE(c && Q && dc, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(H >= 1 && H <= 64, CRF_ERR_UNSUPPORTED, "H=%d outside [1, 64]", H);
    hipLaunchKernelGGL(crf::crf_matrices_bwd_kernel, dim3((unsigned)((H + crf::CMB_ROWS - 1) / crf::CMB_ROWS)), dim3(crf::CMB_BLOCK), 0,
                       crf::as_stream(stream), c, Q, dQ, dP, H, dc);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
