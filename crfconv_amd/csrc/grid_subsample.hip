// Voxel-grid subsampling on gfx950 -- replaces the reference's unordered_map pass
// (utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:5-106) -- for a RAGGED batch of clouds (pos [N, 3] + ptr
// [S + 1]); the host entry crfconv_grid_subsample runs the same launches with one cloud:
//   1. bounds per cloud (sb_bounds_kernel of segment_bounds.hpp: ordered-int atomic minima, and the check of ptr)
//   2. gs_dims: origin and grid dims per cloud in the reference's float ops, and the clouds' key bases
//   3. gs_keys: ONE 64-bit key per point = base[s] + k, k = iX + NX iY + NX NY iZ the reference's voxel key (every op separately
//      rounded), s the point's cloud and base the exclusive scan of the clouds' key ranges: ascending by cloud, then by the
//      reference's voxel key.  A cloud's range is its cell count NX NY NZ, plus `neg` where the float32 origin rounded to above the
//      cloud's minimum: the lowest points then have index -1 (or lower) on that axis, the reference's size_t key wraps around and
//      its rows come LAST in the cloud, so a negative key -d goes to cells + (neg - d), neg = minus the key of the lowest voxel.
//      S > 1 and a cell count or neg past 2^62, or the ranges' sum past 2^64: status SB_OVERFLOW, nothing further runs.
//      S = 1: base = 0, the key is the reference's with its size_t wrap-around, untouched.
//   4. ONE stable radix sort of (key, point id) over all eight bytes
//   5. gs_heads + scan -> voxel ordinal; gs_starts: the voxels' first sorted items, inverse[point] = its voxel's row, and out_ptr --
//      every sorted item writes the entries between its predecessor's cloud and its own (empty clouds repeat an entry), no atomics
//   6. gs_reduce: one thread per (voxel, output column), sums in ARRIVAL order; the thread of column 0 also writes the voxel's count
// Because the sort is stable, each voxel's points are visited in ascending original index, i.e. the order the reference's single pass
// adds them, so barycentres and feature means are bit-exact.  Output rows are cloud by cloud, in ascending voxel key inside a cloud
// (the reference: hash-map iteration order).  Every output word has one writer; the only atomics are those of the bounds pass.
#include "common.hpp"

#include "../../include/crfconv_grid.h"
#include "radix_sort.hpp"
#include "segment_bounds.hpp"

namespace crf {

struct GridDims {
    float org[3];
    float dl;
    unsigned long long NX, NY, NZ;
    unsigned long long base;                               // first key of the cloud
    unsigned long long cells, neg;                         // NX NY NZ; how far below 0 the cloud's voxel keys can reach (S > 1)
};

// float -> size_t as the reference's build converts it (x86-64): values below 2^63 go through the signed conversion, so a negative
// index wraps around -- the origin floor(min / dl) * dl can round to just above the minimum, and the voxel index of the lowest points
// is then -1.  (The device's own float -> unsigned conversion would give 0 there.)
__device__ __forceinline__ unsigned long long gs_cell(float v) {
    return v < 9223372036854775808.f ? (unsigned long long)(long long)v : (unsigned long long)v;
}

enum { GS_VOXELS = 0, GS_STATUS = 1 };                     // the caller's totals[]

// ONE workgroup: origin / grid dims of every cloud with the reference's float arithmetic (grid_subsampling.cpp:27-31), then the bases
// and the status (ws_totals: what the bounds pass left)
__global__ __launch_bounds__(256) void gs_dims_kernel(const unsigned* __restrict__ bnd, const int64_t* __restrict__ ptr, int S, float dl,
                                                      const int64_t* __restrict__ ws_totals, GridDims* __restrict__ gd,
                                                      int64_t* __restrict__ totals) {
    if (ws_totals[SB_STATUS] != 0) {
        if (threadIdx.x == 0) totals[GS_STATUS] = ws_totals[SB_STATUS];
        return;
    }
    __shared__ int s_over;
    if (threadIdx.x == 0) s_over = 0;
    __syncthreads();
    const float inv = __fdiv_rn(1.0f, dl);
    for (int s = threadIdx.x; s < S; s += 256) {
        GridDims g;
        g.dl = dl;
        unsigned long long n[3] = {0ull, 0ull, 0ull}, cells = 0ull, neg = 0ull;
        g.org[0] = g.org[1] = g.org[2] = 0.f;
        if (ptr[s + 1] > ptr[s]) {
            long long lowest[3];                           // the voxel index of the cloud's minimum: 0, or below where the origin rounded up
            for (int a = 0; a < 3; ++a) {
                const float mn = sb_unord(bnd[6 * s + a]), mx = -sb_unord(bnd[6 * s + 3 + a]);
                g.org[a] = mul_rn(floorf(mul_rn(mn, inv)), dl);
                n[a] = gs_cell(floorf(__fdiv_rn(sub_rn(mx, g.org[a]), dl))) + 1ull;
                const float lo = floorf(__fdiv_rn(sub_rn(mn, g.org[a]), dl));
                lowest[a] = lo < 0.f ? (long long)lo : 0ll;
            }
            const unsigned long long xy = n[0] * n[1];
            cells = xy * n[2];
            // the lowest voxel key of the cloud is -neg: indices are monotone in the coordinate, so no point lies below `lowest`
            neg = 0ull - ((unsigned long long)lowest[0] + n[0] * (unsigned long long)lowest[1] + xy * (unsigned long long)lowest[2]);
            const double dneg = -((double)lowest[0] + (double)n[0] * (double)lowest[1] + (double)n[0] * (double)n[1] * (double)lowest[2]);
            // cells and neg below 2^62 each: a key's sign says which side of 0 it is on, and the cloud's key range fits 63 bits
            if (__umul64hi(n[0], n[1]) != 0ull || __umul64hi(xy, n[2]) != 0ull || cells >= (1ull << 62) || !(dneg < 4.0e18)) s_over = 1;
        }
        g.NX = n[0]; g.NY = n[1]; g.NZ = n[2];
        g.cells = cells; g.neg = neg;
        g.base = cells + neg;                              // the cloud's key range (the scan below turns the ranges into the bases)
        gd[s] = g;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long run = 0ull;
    bool over = s_over != 0;
    for (int s = 0; s < S; ++s) {
        const unsigned long long range = gd[s].base;
        gd[s].base = run;
        over |= run + range < run;
        run += range;
    }
    totals[GS_STATUS] = (over && S > 1) ? SB_OVERFLOW : 0;
}

__global__ __launch_bounds__(256) void gs_keys_kernel(const float* __restrict__ pts, int64_t N, const int64_t* __restrict__ ptr, int S,
                                                      const GridDims* __restrict__ gd, const int64_t* __restrict__ totals,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ ids) {
    if (totals[GS_STATUS] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const GridDims g = gd[sb_scene_of(ptr, S, i)];
    const unsigned long long ix = gs_cell(floorf(__fdiv_rn(sub_rn(pts[3 * i + 0], g.org[0]), g.dl)));
    const unsigned long long iy = gs_cell(floorf(__fdiv_rn(sub_rn(pts[3 * i + 1], g.org[1]), g.dl)));
    const unsigned long long iz = gs_cell(floorf(__fdiv_rn(sub_rn(pts[3 * i + 2], g.org[2]), g.dl)));
    unsigned long long k = ix + g.NX * iy + g.NX * g.NY * iz;   // grid_subsampling.cpp:56
    if (S > 1) {
        // a cloud's keys ascend as the reference's size_t keys do: 0 .. cells - 1, then the wrapped negative ones -neg .. -1, in
        // [base, base + cells + neg).  (A key outside that -- positions that are not finite -- is kept inside: clouds never mix.)
        const unsigned long long range = g.cells + g.neg;
        k = (long long)k >= 0 ? k : g.cells + (k + g.neg);
        k = g.base + (k < range ? k : range - 1ull);
    }
    keys[i] = k;
    ids[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void gs_heads_kernel(const unsigned long long* __restrict__ skeys, int64_t N,
                                                       const int64_t* __restrict__ totals, int32_t* __restrict__ head) {
    if (totals[GS_STATUS] != 0) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    head[p] = (p == 0 || skeys[p] != skeys[p - 1]) ? 1 : 0;
}

// per sorted item: the first item of a voxel writes seg_start; every item its point's inverse entry and the out_ptr entries between
// its predecessor's cloud and its own (the last item also those up to S); out_ptr / inverse may be null
__global__ __launch_bounds__(256) void gs_starts_kernel(const int32_t* __restrict__ head, const int32_t* __restrict__ ordinal,
                                                        const uint32_t* __restrict__ sids, int64_t N,
                                                        const int64_t* __restrict__ ptr, int S, int32_t* __restrict__ seg_start,
                                                        int64_t* __restrict__ out_ptr, int64_t* __restrict__ inverse,
                                                        int64_t* __restrict__ totals) {
    if (totals[GS_STATUS] != 0) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int h = head[p], o = ordinal[p];                 // o: the voxels in front of this item
    if (h) seg_start[o] = (int32_t)p;
    if (inverse) inverse[sids[p]] = (int64_t)(o + h - 1);
    const int32_t M = o + h;                               // (at the last item: all voxels)
    if (out_ptr) {
        const int s = sb_scene_of(ptr, S, sids[p]), prev = p ? sb_scene_of(ptr, S, sids[p - 1]) : -1;
        for (int q = prev + 1; q <= s; ++q) out_ptr[q] = o;                    // (s > prev: this item begins a voxel, number o)
        if (p == N - 1)
            for (int q = s + 1; q <= S; ++q) out_ptr[q] = M;
    }
    if (p == N - 1) {
        seg_start[M] = (int32_t)N;
        totals[GS_VOXELS] = M;
    }
}

// One thread per (voxel, output column), the column fastest: columns 0..2 the barycentre, 3..3 + F the feature means, then the L label
// modes.  A workgroup takes G = 256 / W whole voxels (W = 3 + F + L columns; one voxel and a loop over the columns when W > 256), so
// the lanes of a voxel read the same sorted ids and neighbouring words of the same source row.
__global__ __launch_bounds__(256) void gs_reduce_kernel(const float* __restrict__ pts,
                                                        const float* __restrict__ feats, int fdim,
                                                        const int32_t* __restrict__ classes, int ldim, int G, int Wc,
                                                        const uint32_t* __restrict__ sids,
                                                        const int32_t* __restrict__ seg_start,
                                                        const int64_t* __restrict__ totals, int64_t cap,
                                                        float* __restrict__ out_pts,
                                                        float* __restrict__ out_feats,
                                                        int32_t* __restrict__ out_classes, int32_t* __restrict__ counts) {
    if (totals[GS_STATUS] != 0) return;
    const int t = threadIdx.x;
    if (t >= G * Wc) return;
    const int dv = t / Wc, W = 3 + fdim + ldim;
    const int64_t v = (int64_t)blockIdx.x * G + dv;
    const int64_t M = totals[GS_VOXELS];
    if (v >= M || v >= cap) return;
    const int beg = seg_start[v], end = seg_start[v + 1];
    const int n = end - beg;
    for (int c = t - dv * Wc; c < W; c += Wc) {
        if (c < 3) {
            float s = 0.f;
            for (int p = beg; p < end; ++p) s = add_rn(s, pts[3 * (int64_t)sids[p] + c]);
            const float r = (float)(1.0 / (double)n);   // grid_subsampling.cpp:87: double reciprocal narrowed
            out_pts[3 * v + c] = mul_rn(s, r);
            if (c == 0 && counts) counts[v] = n;
        } else if (c < 3 + fdim) {
            const int f = c - 3;
            float acc = 0.f;
            for (int p = beg; p < end; ++p) acc = add_rn(acc, feats[(int64_t)sids[p] * fdim + f]);
            out_feats[v * fdim + f] = __fdiv_rn(acc, (float)n);
        } else {
            const int l = c - 3 - fdim;
            // mode of the column; ties -> smallest label value
            int best = 0, bestc = 0;
            for (int a = beg; a < end; ++a) {
                const int la = classes[(int64_t)sids[a] * ldim + l];
                bool seen = false;
                for (int b = beg; b < a; ++b)
                    if (classes[(int64_t)sids[b] * ldim + l] == la) { seen = true; break; }
                if (seen) continue;
                int cnt = 1;
                for (int b = a + 1; b < end; ++b) cnt += (classes[(int64_t)sids[b] * ldim + l] == la);
                if (cnt > bestc || (cnt == bestc && la < best)) { bestc = cnt; best = la; }
            }
            out_classes[v * ldim + l] = best;
        }
    }
}

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct GsLayout {
    size_t off_totals, off_bnd, off_gd, off_keys, off_skeys, off_ids, off_sids, off_head, off_ord, off_start, off_temp, temp_bytes, total;
};

static GsLayout gs_layout(int64_t N, int64_t S) {
    GsLayout L;
    size_t o = 0;
    L.off_totals = o; o += al(sizeof(int64_t) * 4);        // what sb_bounds_kernel writes its status into
    L.off_bnd = o;   o += al(sizeof(unsigned) * 6 * (size_t)S);
    L.off_gd = o;    o += al(sizeof(GridDims) * (size_t)S);
    L.off_keys = o;  o += al(sizeof(unsigned long long) * N);
    L.off_skeys = o; o += al(sizeof(unsigned long long) * N);
    L.off_ids = o;   o += al(sizeof(uint32_t) * N);
    L.off_sids = o;  o += al(sizeof(uint32_t) * N);
    L.off_head = o;  o += al(sizeof(int32_t) * N);
    L.off_ord = o;   o += al(sizeof(int32_t) * N);
    L.off_start = o; o += al(sizeof(int32_t) * (N + 1));
    // scratch of this library's radix sort (radix_sort.hpp) and of the scan over the voxel heads (scan.hpp)
    const size_t t1 = rsort_workspace(N), t2 = sizeof(int32_t) * scan_block_sums(N) + 256;
    L.temp_bytes = t1 > t2 ? t1 : t2;
    L.off_temp = o;  o += al(L.temp_bytes);
    L.total = o + 256;
    return L;
}

constexpr int64_t GS_MAX = ((int64_t)1 << 31) - 1;

// The launches of both entries: everything is enqueued on `stream`, nothing is read back.  totals [2] on the device.
static int gs_enqueue(const float* points, int64_t N, const int64_t* ptr, int64_t S, const float* feats, int fdim, const int32_t* classes,
                      int ldim, float sampleDl, int64_t cap, void* workspace, size_t workspace_bytes, float* out_points, float* out_feats,
                      int32_t* out_classes, int64_t* out_ptr, int64_t* inverse, int32_t* counts, int64_t* totals, crf_stream_t stream) {
    CRF_REQUIRE(points && ptr && out_points && workspace && totals, CRF_ERR_ARG, "grid_subsample: null pointer");
    CRF_REQUIRE(N > 0 && N <= GS_MAX && S > 0 && S <= GS_MAX, CRF_ERR_ARG, "grid_subsample: N=%lld, S=%lld out of range", (long long)N,
                (long long)S);
    CRF_REQUIRE(sampleDl > 0.f, CRF_ERR_ARG, "sampleDl must be positive");
    CRF_REQUIRE(fdim >= 0 && ldim >= 0 && (!feats || (fdim > 0 && out_feats)) && (!classes || (ldim > 0 && out_classes)), CRF_ERR_ARG,
                "feature / class buffers inconsistent");
    if (!feats) fdim = 0;
    if (!classes) ldim = 0;
    CRF_REQUIRE(cap >= 0, CRF_ERR_ARG, "grid_subsample: cap=%lld is negative", (long long)cap);
    const GsLayout L = gs_layout(N, S);
    CRF_REQUIRE(workspace_bytes >= L.total, CRF_ERR_WORKSPACE, "grid_subsample workspace %zu < %zu",
                workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int64_t* ws_totals = reinterpret_cast<int64_t*>(ws + L.off_totals);
    unsigned* bnd = reinterpret_cast<unsigned*>(ws + L.off_bnd);
    GridDims* gd = reinterpret_cast<GridDims*>(ws + L.off_gd);
    auto* keys = reinterpret_cast<unsigned long long*>(ws + L.off_keys);
    auto* skeys = reinterpret_cast<unsigned long long*>(ws + L.off_skeys);
    uint32_t* ids = reinterpret_cast<uint32_t*>(ws + L.off_ids);
    uint32_t* sids = reinterpret_cast<uint32_t*>(ws + L.off_sids);
    int32_t* head = reinterpret_cast<int32_t*>(ws + L.off_head);
    int32_t* ord = reinterpret_cast<int32_t*>(ws + L.off_ord);
    int32_t* seg_start = reinterpret_cast<int32_t*>(ws + L.off_start);
    void* temp = ws + L.off_temp;

    CRF_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
    CRF_HIP(hipMemsetAsync(ws_totals, 0, 4 * sizeof(int64_t), st));
    CRF_HIP(hipMemsetAsync(bnd, 0xff, sizeof(unsigned) * 6 * (size_t)S, st));
    hipLaunchKernelGGL(sb_bounds_kernel<0>, dim3((unsigned)cdiv(N, SB_BOUNDS_PPB)), dim3(256), 0, st, points, N, ptr, (int)S, bnd, ws_totals);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_dims_kernel, dim3(1), dim3(256), 0, st, bnd, ptr, (int)S, sampleDl, ws_totals, gd, totals);
    CRF_LAUNCH_CHECK();
    const dim3 flat((unsigned)cdiv(N, 256));
    hipLaunchKernelGGL(gs_keys_kernel, flat, dim3(256), 0, st, points, N, ptr, (int)S, gd, totals, keys, ids);
    CRF_LAUNCH_CHECK();
    // stable sort of (voxel key, point id): points of a voxel stay in arrival order (grid_subsampling.cpp:58-63 sums in that order).
    // All eight digits are sorted: how many key bits are in use is device data (GridDims), and a pass whose digit is the same for
    // every point costs 32 B per point -- less than reading the answer back would
    if (rsort_pairs_u64(keys, ids, skeys, sids, N, 0, 64, temp, st) == 0) {
        auto* tk = keys; keys = skeys; skeys = tk;           // (eight passes end in the first pair of buffers)
        auto* ti = ids; ids = sids; sids = ti;
    }
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_heads_kernel, flat, dim3(256), 0, st, skeys, N, totals, head);
    CRF_LAUNCH_CHECK();
    exclusive_scan_i32(head, ord, N, reinterpret_cast<int32_t*>(temp), st);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(gs_starts_kernel, flat, dim3(256), 0, st, head, ord, sids, N, ptr, (int)S, seg_start, out_ptr, inverse, totals);
    CRF_LAUNCH_CHECK();
    // the reduce kernel reads M from device memory; launch for the worst case (M <= min(N, cap) rows written)
    const int64_t rows = N < cap ? N : cap;
    if (rows > 0) {
        const int W = 3 + fdim + ldim, Wc = W < 256 ? W : 256, G = 256 / Wc;
        hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)cdiv(rows, G)), dim3(256), 0, st, points, feats, fdim, classes, ldim, G, Wc,
                           sids, seg_start, totals, cap, out_points, out_feats, out_classes, counts);
        CRF_LAUNCH_CHECK();
    }
    return CRF_OK;
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_grid_subsample_segments_workspace(int64_t N, int64_t S) {
    if (N < 1 || N > GS_MAX || S < 1 || S > GS_MAX) return 0;
    return gs_layout(N, S).total;
}

extern "C" int crfconv_grid_subsample_segments(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const float* feats, int F,
                                               const int32_t* labels, int L, float size, int64_t cap, void* workspace,
                                               size_t workspace_bytes, float* out_pos, float* out_feats, int32_t* out_labels,
                                               int64_t* out_ptr, int64_t* inverse, int32_t* counts, int64_t* totals, crf_stream_t stream) {
    return gs_enqueue(pos, N, ptr, S, feats, F, labels, L, size, cap, workspace, workspace_bytes, out_pos, out_feats, out_labels, out_ptr,
                      inverse, counts, totals, stream);
}

extern "C" int64_t crfconv_grid_subsample(const float* points, int64_t N, const float* feats, int fdim,
                                          const int32_t* classes, int ldim, float sampleDl,
                                          float* out_points, float* out_feats, int32_t* out_classes,
                                          int64_t cap) {
    CRF_REQUIRE(points && out_points, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(N > 0, CRF_ERR_ARG, "empty cloud");
    if (cap > N) cap = N;
    CRF_REQUIRE(N <= GS_MAX, CRF_ERR_ARG, "N=%lld out of range", (long long)N);
    // one cloud: ptr = {0, N} and the totals sit behind the workspace proper
    const size_t wsb = gs_layout(N, 1).total;
    const int64_t h_ptr[2] = {0, N};
    int64_t h_totals[2] = {0, 0};
    int64_t* d_tail = nullptr;
    float *dp = nullptr, *df = nullptr, *dop = nullptr, *dof = nullptr;
    int32_t *dc = nullptr, *doc = nullptr;
    void* ws = nullptr;
    int64_t rc = CRF_OK;
    hipError_t e;
#define TRY(x) if ((e = (x)) != hipSuccess) { set_error("%s: %s", #x, hipGetErrorString(e)); rc = CRF_ERR_HIP; goto done; }
    TRY(hipMalloc(&dp, sizeof(float) * 3 * N));
    TRY(hipMalloc(&dop, sizeof(float) * 3 * cap));
    TRY(hipMemcpy(dp, points, sizeof(float) * 3 * N, hipMemcpyHostToDevice));
    if (feats) {
        TRY(hipMalloc(&df, sizeof(float) * fdim * N));
        TRY(hipMalloc(&dof, sizeof(float) * fdim * cap));
        TRY(hipMemcpy(df, feats, sizeof(float) * fdim * N, hipMemcpyHostToDevice));
    }
    if (classes) {
        TRY(hipMalloc(&dc, sizeof(int32_t) * ldim * N));
        TRY(hipMalloc(&doc, sizeof(int32_t) * ldim * cap));
        TRY(hipMemcpy(dc, classes, sizeof(int32_t) * ldim * N, hipMemcpyHostToDevice));
    }
    TRY(hipMalloc(&ws, wsb + 4 * sizeof(int64_t)));
    d_tail = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + wsb);
    TRY(hipMemcpy(d_tail, h_ptr, sizeof(h_ptr), hipMemcpyHostToDevice));
    rc = gs_enqueue(dp, N, d_tail, 1, df, fdim, dc, ldim, sampleDl, cap, ws, wsb, dop, dof, doc, nullptr, nullptr, nullptr, d_tail + 2,
                    nullptr);
    if (rc < 0) goto done;
    TRY(hipMemcpy(h_totals, d_tail + 2, sizeof(h_totals), hipMemcpyDeviceToHost));      // (waits for the launches)
    rc = h_totals[GS_VOXELS];
    if (rc > cap) {
        set_error("grid_subsample: %lld voxels but capacity %lld", (long long)rc, (long long)cap);
        rc = CRF_ERR_WORKSPACE;
        goto done;
    }
    TRY(hipMemcpy(out_points, dop, sizeof(float) * 3 * rc, hipMemcpyDeviceToHost));
    if (feats) TRY(hipMemcpy(out_feats, dof, sizeof(float) * fdim * rc, hipMemcpyDeviceToHost));
    if (classes) TRY(hipMemcpy(out_classes, doc, sizeof(int32_t) * ldim * rc, hipMemcpyDeviceToHost));
#undef TRY
done:
    if (dp) (void)hipFree(dp);
    if (df) (void)hipFree(df);
    if (dc) (void)hipFree(dc);
    if (dop) (void)hipFree(dop);
    if (dof) (void)hipFree(dof);
    if (doc) (void)hipFree(doc);
    if (ws) (void)hipFree(ws);
    return rc;
}
