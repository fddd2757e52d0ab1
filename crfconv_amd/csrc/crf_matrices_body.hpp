// The forward of the CRF layers' two loop-invariant matrices as a device function over caller-provided LDS, so that its workgroups can
// run as a launch of their own (crf_matrices.hip: crf_matrices_batched_kernel, one layer being a batch of one) or ride along in a long launch whose
// inputs do not depend on them (pointconv.hip: the first PointConv's statistics pass, crfconv_pointconv_uvstats_hosting).  The same for
// the backward: crf_matrices_bwd_slab and its job table (crf_matrices_bwd_jobs) serve crf_matrices.hip's own launches and the
// end-of-pass dW launch that carries the slabs (mlp_bwd.hip: mlp_dw_jobs_hosting_kernel).
#pragma once
#include "common.hpp"

namespace crf {

// The two loop-invariant matrices of a CRF layer from its compatibility factor c [H, H] in one launch:
//   Q = (I + c^T c)^-1,   P = c^T c Q = I - Q            (continuous_crf_conv_big.py:67-72)
// The 64 pivots of the Gauss-Jordan sweep are sequential, and what a pivot costs is the INSTRUCTIONS every wavefront issues
// around its handful of float64 multiply-adds (barrier, LDS traffic, the reciprocal, the selects that treat pivot row /
// column / element apart) -- round 3's 1024-thread form (2 x 2 tiles, sixteen wavefronts on one CU) took 35 us for the four
// layers of PointConvBig.  This form: 256 threads, a 4 x 4 cyclic tile each (one wavefront per SIMD: the per-pivot overhead is
// paid once per SIMD, not four times), the pivot row and column in LDS in TILE-MAJOR order (a thread's four values are one
// 32-byte segment), 1 / pivot by the hardware estimate + two Newton steps, and NO special cases in the update: with
//   col'[p] = pivot - 1  (threads that own the pivot row)      row'[p] = 1 + 1 / pivot  (threads that own the pivot column)
// the one fused multiply-add  t -= col' * row'  leaves row * (1 / pivot) in the pivot row, -col / pivot in the pivot column and
// 1 / pivot in the pivot itself (pivot * (1 / pivot) = 1 up to float64 rounding).
constexpr int CMF_BLOCK = 256;
constexpr int CMF_LDS_BYTES = 4 * 64 * (int)sizeof(double) + 64 * 65 * (int)sizeof(float);      // pivot row / column (two parities each) | c, stride 65
__device__ __forceinline__ void gauss_jordan_fma(double (&t)[4][4], int H, double (*s_row)[64], double (*s_col)[64]) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {                     // pivot p = 16 ip + pp lives in local row / column ip
        for (int pp = 0; pp < 16; ++pp) {
            const int p = 16 * ip + pp;
            if (p >= H) break;                           // uniform: rows beyond H are identity already
            const int b = p & 1;
            if (tr == pp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s_row[b][4 * tc + j] = t[ip][j];       // column tc + 16 j of row p
            }
            if (tc == pp) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s_col[b][4 * tr + i] = t[i][ip];       // row tr + 16 i of column p
            }
            __syncthreads();
            const double pv = s_row[b][4 * pp + ip];                              // element (p, p)
            double piv = __builtin_amdgcn_rcp(pv);
            piv = fma(piv, fma(-pv, piv, 1.0), piv);
            piv = fma(piv, fma(-pv, piv, 1.0), piv);
            double rowv[4], colv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) rowv[j] = s_row[b][4 * tc + j] * piv;
#pragma unroll
            for (int i = 0; i < 4; ++i) colv[i] = s_col[b][4 * tr + i];
            if (tc == pp) rowv[ip] = 1.0 + piv;
            if (tr == pp) colv[ip] = pv - 1.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) t[i][j] = fma(-colv[i], rowv[j], t[i][j]);
        }
    }
}
__device__ __forceinline__ void crf_matrices_body(const float* __restrict__ cmat, int H,
                                                  float* __restrict__ Qout, float* __restrict__ Pout, char* __restrict__ lds /*CMF_LDS_BYTES, 16-byte aligned*/) {
    double (*s_row)[64] = reinterpret_cast<double (*)[64]>(lds);
    double (*s_col)[64] = reinterpret_cast<double (*)[64]>(lds + 2 * 64 * sizeof(double));
    float* s_c = reinterpret_cast<float*>(lds + 4 * 64 * sizeof(double));
    for (int e = threadIdx.x; e < 64 * 65; e += CMF_BLOCK) s_c[e] = 0.f;           // columns >= H of c: zero (M stays identity there)
    __syncthreads();
    for (int e = threadIdx.x; e < H * H; e += CMF_BLOCK) s_c[(e / H) * 65 + (e % H)] = cmat[e];
    __syncthreads();
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    double t[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) t[i][j] = (tr + 16 * i == tc + 16 * j) ? 1.0 : 0.0;
    for (int k = 0; k < H; ++k) {                        // M = I + c^T c: eight LDS reads feed sixteen multiply-adds
        double a[4], bq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = (double)s_c[k * 65 + tr + 16 * i];
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = (double)s_c[k * 65 + tc + 16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t[i][j] = fma(a[i], bq[j], t[i][j]);
    }
    gauss_jordan_fma(t, H, s_row, s_col);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tr + 16 * i, c = tc + 16 * j;
            if (r < H && c < H) {
                Qout[r * H + c] = (float)t[i][j];
                Pout[r * H + c] = (float)((r == c ? 1.0 : 0.0) - t[i][j]);
            }
        }
}


// All CRF layers of a network in ONE launch (one workgroup each): the Gauss-Jordan sweep is a latency chain of ~20 us
// whatever H is, so four layers cost what one does.
constexpr int CM_MAX = 8;
struct CrfMatJobs {
    const float* c[CM_MAX];
    const float* Q_in[CM_MAX];
    const float* gQ[CM_MAX];
    const float* gP[CM_MAX];
    float* Q[CM_MAX];
    float* P[CM_MAX];
    float* dc[CM_MAX];
    int H[CM_MAX];
    int slab_base[CM_MAX + 1];                     // backward: prefix of ceil(H / CMB_ROWS) -- first workgroup of each layer
};

// dc from dQ and dP (either may be NULL = zero).  With D = dQ - dP (P = I - Q), M = I + c^T c:
//   dM = -Q^T D Q^T,   dc = c (dM + dM^T) = -c (S + S^T),   S = Q^T D Q^T.
// Q is symmetric (the inverse of a symmetric matrix; its float rounding included, to ~1e-8), so S + S^T = Q (D + D^T) Q and
//   dc = -((c Q) (D + D^T)) Q
// is a chain of three products in which every ROW of the result depends on the same row of c only: a workgroup takes a slab
// of CMB_ROWS rows through all three products without ever meeting another workgroup (H / CMB_ROWS workgroups per layer,
// float64 accumulation, operands as float in LDS).  The one-workgroup form (T = Q^T D, S = T Q^T, c (S + S^T): three full
// H^3 float64 products on 1024 threads of ONE CU, 35 us for the four layers of PointConvBig) was instruction-bound.
constexpr int CMB_ROWS = 8, CMB_BLOCK = CMB_ROWS * 64;
__device__ __forceinline__ void crf_matrices_bwd_slab(const float* __restrict__ cmat, const float* __restrict__ Q,
                                                      const float* __restrict__ dQ, const float* __restrict__ dP,
                                                      int H, int row0, float* __restrict__ dc) {
    __shared__ float s_q[64 * 65], s_d[64 * 65];
    __shared__ double s_t[2][CMB_ROWS][65];
    for (int e = threadIdx.x; e < H * H; e += (int)blockDim.x) {              // (a rider in a launch of larger workgroups: mlp_dw_jobs_hosting_kernel)
        const int r = e / H, c = e % H;
        s_q[r * 65 + c] = Q[e];
        s_d[r * 65 + c] = (dQ ? dQ[e] : 0.f) - (dP ? dP[e] : 0.f);            // D
    }
    const int r = (threadIdx.x >> 6) & (CMB_ROWS - 1), j = threadIdx.x & 63, row = row0 + r;
    const bool live = (int)threadIdx.x < CMB_BLOCK && row < H && j < H;
    if (live) s_t[0][r][j] = (double)cmat[row * H + j];
    __syncthreads();
    double acc = 0.0;
    if (live)
        for (int k = 0; k < H; ++k) acc += s_t[0][r][k] * (double)s_q[k * 65 + j];                 // (c Q)[row][j]
    if (live) s_t[1][r][j] = acc;
    __syncthreads();
    acc = 0.0;
    if (live)
        for (int k = 0; k < H; ++k) acc += s_t[1][r][k] * ((double)s_d[k * 65 + j] + (double)s_d[j * 65 + k]);   // . (D + D^T)
    if (live) s_t[0][r][j] = acc;
    __syncthreads();
    acc = 0.0;
    if (live) {
        for (int k = 0; k < H; ++k) acc += s_t[0][r][k] * (double)s_q[k * 65 + j];                 // . Q
        dc[row * H + j] = (float)(-acc);
    }
}

}  // namespace crf

// host side: the backward's job table from the entry points' arrays, checked (nslab = workgroups of the slabs)
static int crf_matrices_bwd_jobs(const float* const* c, const float* const* Q, const float* const* gQ, const float* const* gP, const int* H, int n,
                                 float* const* dc, crf::CrfMatJobs& j, int& nslab) {
    CRF_REQUIRE(c && Q && gQ && gP && H && dc && n >= 1 && n <= crf::CM_MAX, CRF_ERR_ARG, "null pointer or n=%d outside [1, %d]", n, crf::CM_MAX);
    j = crf::CrfMatJobs();
    for (int i = 0; i < n; ++i) {
        CRF_REQUIRE(c[i] && Q[i] && dc[i] && H[i] >= 1 && H[i] <= 64, CRF_ERR_ARG, "job %d: null pointer or H=%d outside [1, 64]", i, H[i]);
        j.c[i] = c[i]; j.Q_in[i] = Q[i]; j.gQ[i] = gQ[i]; j.gP[i] = gP[i]; j.dc[i] = dc[i]; j.H[i] = H[i];
        j.slab_base[i + 1] = j.slab_base[i] + (H[i] + crf::CMB_ROWS - 1) / crf::CMB_ROWS;
    }
    nslab = j.slab_base[n];
    for (int i = n; i < crf::CM_MAX; ++i) j.slab_base[i + 1] = 0x7fffffff;      // (never reached by a block index)
    return CRF_OK;
}
