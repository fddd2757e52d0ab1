// Exact batched kNN on gfx950 -- replaces the reference's nanoflann KD-tree extension
// (utils/nearest_neighbors/knn_.cxx:22-135, knn_.h:2-19) with three searches that rank the same keys (crfconv_knn_batch_dev says
// which serves which (npts, K)):
//   whole cloud   knn_brute_kernel: small clouds, no grid; sixteen lanes per query look at every point of the cloud.
//   uniform grid, built by
//     1. per-cloud bounding box            (one block per cloud)
//     2. cell id + histogram               (flat, int atomics)
//     3. exclusive scan of cell counts     (scan.hpp: this library's own scratch-free scan)
//     4. counting-sort scatter             (points packed as float4 {x, y, z, id})
//   and searched over expanding Chebyshev rings of cells until the K-th distance is strictly inside the searched cube, by
//     5.  knn_query_kernel: one lane per query, register-resident top-K, or
//     5b. knn_coop_kernel: sixteen lanes per query, the ring's row segments dealt over them, top-K in an LDS pool.
// Result contract (bit-exact against the oracle / the reference on tie-free input):
//   distance = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) in float32, no FMA contraction
//   (nanoflann.hpp:342-347); neighbours ascending by (distance, point id).
// The grid build and both grid searches are ONE family over two descriptions of "which rows are cloud b" (a Split):
//   UniformSplit  B clouds of npts points and nq queries each, blockIdx.y = cloud, everything arithmetic (crfconv_knn_batch_dev);
//   RaggedSplit   a ragged batch: row boundaries, grid resolutions and cell bases live in DEVICE arrays that segments_kernel
//                 derives from pts_ptr / q_ptr, one flat launch over all rows (crfconv_knn_segments_dev).
#include "common.hpp"

#include <algorithm>
#include <cstdlib>
#include "scan.hpp"

namespace crf {

struct GridInfo {  // one per cloud, device resident
    float ox, oy, oz;   // origin (bbox min)
    float cell, inv;    // cell edge, 1 / cell
    int nx, ny, nz;
    float margin;       // absolute safety margin for the stop test
};

constexpr int QBLOCK = 128;

__device__ __forceinline__ float sqdist_exact(float qx, float qy, float qz, float px, float py, float pz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
}

// ------------------------------------------------------------------ which rows are cloud b
struct Row {            // one point or query row
    bool live;          // inside a cloud
    int b;              // its cloud
    int64_t row, local; // row of the whole array; row within the cloud
};

struct UniformSplit {
    static constexpr bool RAGGED = false;
    int64_t npts, nq;
    int ncell_alloc, G0;
    // x = blockIdx.x * block + offset, the cloud is blockIdx.y
    __device__ __forceinline__ Row point(int64_t x) const { const int b = blockIdx.y; return {x < npts, b, (int64_t)b * npts + x, x}; }
    __device__ __forceinline__ Row query(int64_t x) const { const int b = blockIdx.y; return {x < nq, b, (int64_t)b * nq + x, x}; }
    __device__ __forceinline__ int64_t queries_x() const { return nq; }
    __device__ __forceinline__ void cloud(int b, int64_t& p0, int64_t& n, int& g0) const { p0 = (int64_t)b * npts; n = npts; g0 = G0; }
    __device__ __forceinline__ int64_t cell0(int b) const { return (int64_t)b * ncell_alloc; }
    __device__ __forceinline__ int id0(int) const { return 0; }                 // output ids are local to the cloud
};

// Grid resolution of a cloud of n points: the largest g in [1, 160] with 0.6 g^3 <= n (grid_g0's rule, 0.6 points per cell, in
// integers so that the device and the host's workspace bound agree on every n).
__host__ __device__ inline int seg_g0(int64_t n) {
    int g = 1;
    while (g < 160 && 3ll * (g + 1) * (g + 1) * (g + 1) <= 5ll * n) ++g;
    return g;
}
__host__ __device__ inline int seg_cells(int64_t n) { const int g = seg_g0(n) + 1; return g * g * g; }

// The segment s with b[s] <= x < b[s + 1], or -1.  b [S + 1] is a boundary array that segments_kernel wrote: ascending, inside
// [0, total].  Bounds / termination: at most log2(S + 2) <= 17 probes of b[0 .. S], whatever b holds.
__device__ __forceinline__ int segment_of(const int32_t* __restrict__ b, int S, int x) {
    int lo = 0, hi = S + 1;                                 // -> the first index whose boundary is above x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (b[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1 < S ? lo - 1 : -1;                        // lo == 0: x in front of the first segment; lo == S + 1: behind the last
}

struct RaggedSplit {
    static constexpr bool RAGGED = true;
    const int32_t *pb, *qb, *cb;        // [S + 1] each: point row, query row and cell boundaries of the segments
    int S, total_pts, total_q;
    // x = blockIdx.x * block + offset is the row itself; rows outside every segment are not live
    __device__ __forceinline__ Row point(int64_t x) const {
        if (x >= total_pts) return {false, 0, 0, 0};
        const int b = segment_of(pb, S, (int)x);
        return {b >= 0, b < 0 ? 0 : b, x, b < 0 ? 0 : x - pb[b]};
    }
    __device__ __forceinline__ Row query(int64_t x) const {
        if (x >= total_q) return {false, 0, 0, 0};
        const int b = segment_of(qb, S, (int)x);
        return {b >= 0, b < 0 ? 0 : b, x, b < 0 ? 0 : x - qb[b]};
    }
    __device__ __forceinline__ int64_t queries_x() const { return total_q; }
    __device__ __forceinline__ void cloud(int b, int64_t& p0, int64_t& n, int& g0) const { p0 = pb[b]; n = pb[b + 1] - pb[b]; g0 = seg_g0(n); }
    __device__ __forceinline__ int64_t cell0(int b) const { return cb[b]; }
    __device__ __forceinline__ int id0(int b) const { return pb[b]; }           // output ids are rows of pts
};

// ------------------------------------------------------------------ 0. (ragged) pts_ptr / q_ptr -> segment boundaries
// ONE block.  pb / qb = the running maximum of the pointer arrays clamped to [0, total]: ascending and in range whatever the
// arrays hold, so the segments are disjoint ranges of rows that exist, and sum(n_s) <= total_pts, which is what the workspace
// bound (seg_cells_bound) needs.  Honest pointer arrays pass through unchanged.  cb = exclusive scan of seg_cells(n_s).
constexpr int SEG_BLOCK = 1024;
template <bool MAX>
__device__ __forceinline__ int block_exclusive(int v, int* s_a, int* s_b) {      // exclusive scan (sum or max, identity 0) over the block
    int* src = s_a;
    int* dst = s_b;
    src[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < SEG_BLOCK; o <<= 1) {
        int t = src[threadIdx.x];
        if ((int)threadIdx.x >= o) { const int u = src[threadIdx.x - o]; t = MAX ? max(t, u) : t + u; }
        dst[threadIdx.x] = t;
        __syncthreads();
        int* w = src; src = dst; dst = w;
    }
    const int r = threadIdx.x > 0 ? src[threadIdx.x - 1] : 0;
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(SEG_BLOCK) void segments_kernel(const int64_t* __restrict__ pts_ptr, const int64_t* __restrict__ q_ptr,
                                                             int S, int total_pts, int total_q, int32_t* __restrict__ pb,
                                                             int32_t* __restrict__ qb, int32_t* __restrict__ cb) {
    __shared__ int s_a[SEG_BLOCK], s_b[SEG_BLOCK];
    const int chunk = (S + 1 + SEG_BLOCK - 1) / SEG_BLOCK;                       // <= 64 consecutive boundaries per thread
    const int i0 = min((int)threadIdx.x * chunk, S + 1), i1 = min(i0 + chunk, S + 1);
    for (int which = 0; which < 2; ++which) {
        const int64_t* ptr = which ? q_ptr : pts_ptr;
        int32_t* out = which ? qb : pb;
        const int64_t total = which ? total_q : total_pts;
        int m = 0;
        for (int i = i0; i < i1; ++i) m = max(m, (int)min(max(ptr[i], (int64_t)0), total));   // bounds: clamped BEFORE any use
        int run = block_exclusive<true>(m, s_a, s_b);
        for (int i = i0; i < i1; ++i) { run = max(run, (int)min(max(ptr[i], (int64_t)0), total)); out[i] = run; }
    }
    __syncthreads();                                        // pb[i1] may be another thread's
    int cells = 0;
    for (int i = i0; i < min(i1, S); ++i) cells += seg_cells(pb[i + 1] - pb[i]);
    int run = block_exclusive<false>(cells, s_a, s_b);
    for (int i = i0; i < i1; ++i) { cb[i] = run; if (i < S) run += seg_cells(pb[i + 1] - pb[i]); }
}

// ------------------------------------------------------------------ 1. bounding box -> grid
constexpr float SEG_COORD_MAX = 1e18f;      // ragged form: coordinates beyond it (and NaN) stay out of the box; such points land in border cells
template <class Split>
__global__ __launch_bounds__(1024) void bbox_kernel(const float* __restrict__ pts, const Split split,
                                                    GridInfo* __restrict__ info) {
    int64_t p0, npts;
    int G0;
    split.cloud(blockIdx.x, p0, npts, G0);
    const float* p = pts + p0 * 3;
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int64_t i = threadIdx.x; i < npts; i += 1024) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = p[3 * i + a];
            if constexpr (Split::RAGGED) { if (!(fabsf(v) <= SEG_COORD_MAX)) continue; }
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
    __shared__ float smn[16][3], smx[16][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float lo = mn[a], hi = mx[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, WAVE));
            hi = fmaxf(hi, __shfl_xor(hi, o, WAVE));
        }
        if (lane == 0) { smn[wave][a] = lo; smx[wave][a] = hi; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = smn[0][a]; hi[a] = smx[0][a];
            for (int w = 1; w < 16; ++w) { lo[a] = fminf(lo[a], smn[w][a]); hi[a] = fmaxf(hi[a], smx[w][a]); }
            if constexpr (Split::RAGGED) { if (!(lo[a] <= hi[a])) lo[a] = hi[a] = 0.f; }      // no point, or none with a usable coordinate
        }
        const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
        float emax = fmaxf(ex, fmaxf(ey, ez));
        if (!(emax > (Split::RAGGED ? 1e-30f : 0.f))) emax = 1.f;  // all points coincide (or a single point); ragged: 1 / cell stays finite
        GridInfo g;
        g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2];
        g.cell = emax / (float)G0;
        g.inv = 1.0f / g.cell;
        g.nx = min(G0, (int)(ex * g.inv)) + 1;
        g.ny = min(G0, (int)(ey * g.inv)) + 1;
        g.nz = min(G0, (int)(ez * g.inv)) + 1;      // ragged: 0 <= e * inv <= G0 (1 + eps) and finite by the two guards above, so 1 <= n <= G0 + 1
        const float amax = fmaxf(fmaxf(fabsf(lo[0]), fabsf(hi[0])),
                                 fmaxf(fmaxf(fabsf(lo[1]), fabsf(hi[1])), fmaxf(fabsf(lo[2]), fabsf(hi[2]))));
        g.margin = 1e-5f * (amax + emax) + 1e-30f;
        info[blockIdx.x] = g;
    }
}

// SAFE (the ragged form): the same cell for every finite coordinate, and a cell of the grid for NaN / infinite ones too -- the
// comparisons decide before any float -> int conversion, so nothing rests on how an out-of-range conversion behaves.
template <bool SAFE>
__device__ __forceinline__ int3 cell_of(const GridInfo& g, float x, float y, float z) {
    if constexpr (SAFE) {
        const float tx = (x - g.ox) * g.inv, ty = (y - g.oy) * g.inv, tz = (z - g.oz) * g.inv;
        return make_int3(tx >= 0.f ? (tx < (float)g.nx ? (int)tx : g.nx - 1) : 0, ty >= 0.f ? (ty < (float)g.ny ? (int)ty : g.ny - 1) : 0,
                         tz >= 0.f ? (tz < (float)g.nz ? (int)tz : g.nz - 1) : 0);
    }
    int cx = (int)floorf((x - g.ox) * g.inv), cy = (int)floorf((y - g.oy) * g.inv),
        cz = (int)floorf((z - g.oz) * g.inv);
    cx = min(max(cx, 0), g.nx - 1);
    cy = min(max(cy, 0), g.ny - 1);
    cz = min(max(cz, 0), g.nz - 1);
    return make_int3(cx, cy, cz);
}

__global__ __launch_bounds__(256) void zero_kernel(uint4* __restrict__ p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------ 2. histogram
template <class Split>
__global__ __launch_bounds__(256) void cell_count_kernel(const float* __restrict__ pts, const Split split,
                                                         const GridInfo* __restrict__ info,
                                                         int32_t* __restrict__ cell_id,
                                                         int32_t* __restrict__ counts) {
    const Row r = split.point((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (!r.live) return;                        // ragged: a row of no segment is in no cell, and cell_scatter_kernel asks again
    const GridInfo g = info[r.b];
    const float* p = pts + r.row * 3;
    const int3 c = cell_of<Split::RAGGED>(g, p[0], p[1], p[2]);
    const int cid = (c.z * g.ny + c.y) * g.nx + c.x;    // bounds: < nx ny nz <= (G0 + 1)^3, the cells bbox_kernel's cloud owns from cell0
    cell_id[r.row] = cid;
    atomicAdd(&counts[split.cell0(r.b) + cid], 1);
}

// ------------------------------------------------------------------ 4. scatter
template <class Split>
__global__ __launch_bounds__(256) void cell_scatter_kernel(const float* __restrict__ pts, const Split split,
                                                           const int32_t* __restrict__ cell_id,
                                                           const int32_t* __restrict__ starts,
                                                           int32_t* __restrict__ fill,
                                                           float4* __restrict__ sorted) {
    const Row r = split.point((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (!r.live) return;
    const int64_t g = r.row;
    const int64_t c = split.cell0(r.b) + cell_id[g];
    // bounds: starts is the scan of the counts of exactly these rows, so pos < (number of live rows) <= total points
    const int pos = starts[c] + atomicAdd(&fill[c], 1);
    sorted[pos] = make_float4(pts[3 * g], pts[3 * g + 1], pts[3 * g + 2], __int_as_float((int)r.local));
}

// ------------------------------------------------------------------ 5. query
// Candidates are ranked by ONE 64-bit key = (float32 distance bits << 32) | point id: squared distances are
// non-negative, so their bit patterns order like the values, and the key order is exactly (distance, id).
__device__ __forceinline__ unsigned long long knn_key(float d, int id) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)id;
}
constexpr unsigned long long KNN_KEY_INF = ((unsigned long long)0x7f800000u << 32) | 0x7fffffffu;

template <int KM>
struct TopK {
    unsigned long long key[KM];     // ascending
    // Only K <= KM slots are live: the first KM - K are pinned at key 0 (nothing is < 0, so nothing displaces them)
    // and the live ones end at the static position KM - 1 (a runtime "key[K - 1]" would push the array to scratch).
    __device__ __forceinline__ void init(int K) {
#pragma unroll
        for (int k = 0; k < KM; ++k) key[k] = (k < KM - K) ? 0ull : KNN_KEY_INF;
    }
    __device__ __forceinline__ unsigned long long kth_key() const { return key[KM - 1]; }
    __device__ __forceinline__ float kth() const { return __uint_as_float((unsigned int)(key[KM - 1] >> 32)); }
    __device__ __forceinline__ void offer(unsigned long long c) {
        if (!(c < key[KM - 1])) return;
        // sorted insert with selects only (static register indices, no conditional stores)
        bool below = c < key[KM - 1];                       // c < key[k], carried down the slots
#pragma unroll
        for (int k = KM - 1; k > 0; --k) {
            const bool below_prev = c < key[k - 1];         // slot k takes its upper neighbour
            key[k] = below_prev ? key[k - 1] : (below ? c : key[k]);
            below = below_prev;
        }
        key[0] = below ? c : key[0];
    }
};

constexpr int QCAP = 8;     // accepted candidates a lane may hold before the wavefront inserts them
constexpr Widths<1, 32, 64> KNN_QUERY_CAPS{};       // top-K capacities KM the one-lane search is compiled for (K <= KM)

template <int KM, class Split>
__global__ __launch_bounds__(QBLOCK) void knn_query_kernel(const float* __restrict__ queries, const Split split, int K,
                                                           const GridInfo* __restrict__ info,
                                                           const int32_t* __restrict__ starts,
                                                           const float4* __restrict__ sorted,
                                                           int64_t* __restrict__ out64,
                                                           int32_t* __restrict__ out32) {
    // The sorted insert is a ~100-instruction select chain and a wavefront runs it whenever ANY of its 64 queries
    // accepts a candidate -- with independent queries that is nearly every candidate.  Accepted keys are therefore
    // parked in a per-lane LDS queue (a cheap predicated store) and inserted in wave-wide batches: when some lane's
    // queue is full, and at the end of every ring (the stop test needs the true K-th distance).
    constexpr bool QUEUED = KM > 1;
    __shared__ unsigned long long s_queue[QUEUED ? QCAP * QBLOCK : 1];
    const int64_t x = (int64_t)blockIdx.x * QBLOCK + threadIdx.x;
    if (x >= split.queries_x()) return;
    const Row row = split.query(x);
    const int64_t o = row.row * K;
    if constexpr (Split::RAGGED) {
        if (!row.live) {                                    // a query of no segment has no neighbours
            for (int k = 0; k < K; ++k) {
                if (out64) out64[o + k] = -1;
                if (out32) out32[o + k] = -1;
            }
            return;
        }
    }
    const int b = row.b;
    const GridInfo g = info[b];
    const float* qp = queries + row.row * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const int3 c = cell_of<Split::RAGGED>(g, qx, qy, qz);
    const int32_t* st = starts + split.cell0(b);
    const int id0 = split.id0(b);

    TopK<KM> best;
    best.init(K);
    int cnt = 0;
    unsigned long long bound = KNN_KEY_INF;                 // K-th key as of the last flush (only ever too large)
    auto flush = [&]() {
        if constexpr (QUEUED) {
            for (int i = 0; i < QCAP; ++i) {
                if (!__any(i < cnt)) break;
                if (i < cnt) best.offer(s_queue[i * QBLOCK + threadIdx.x]);
            }
            cnt = 0;
            bound = best.kth_key();
        }
    };
    auto consider = [&](const float4 s) {
        const unsigned long long key = knn_key(sqdist_exact(qx, qy, qz, s.x, s.y, s.z), __float_as_int(s.w));
        if constexpr (QUEUED) {
            if (key < bound) {
                s_queue[cnt * QBLOCK + threadIdx.x] = key;
                ++cnt;
            }
            if (__any(cnt == QCAP)) flush();
        } else {
            best.offer(key);
        }
    };
    // Termination: r, z, y and x run over the grid's extent (n <= 161 per axis) and p over candidate ranges inside the cloud's
    // part of `sorted` -- none of the bounds depends on how many neighbours were found or on the query's coordinates, so a cloud
    // with fewer than K points (the ragged form; the K-th key stays infinite, the stop test below never holds) ends at the ring
    // whose cube covers the grid, and a NaN / infinite query (every gap comparison false, or an infinite gap) ends no later.
    const int rmax = max(g.nx, max(g.ny, g.nz));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(c.z - r, 0), z1 = min(c.z + r, g.nz - 1);
        const int y0 = max(c.y - r, 0), y1 = min(c.y + r, g.ny - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = (z == c.z - r) || (z == c.z + r);
            for (int y = y0; y <= y1; ++y) {
                const bool full = zface || (y == c.y - r) || (y == c.y + r);
                // full: whole x-span of the shell row; otherwise only its two end cells
                const int nseg = full ? 1 : (r == 0 ? 1 : 2);
                for (int sgi = 0; sgi < nseg; ++sgi) {
                    int xa, xb;
                    if (full) { xa = max(c.x - r, 0); xb = min(c.x + r, g.nx - 1); }
                    else if (sgi == 0) { xa = xb = c.x - r; }
                    else { xa = xb = c.x + r; }
                    if (xa < 0 || xb >= g.nx || xa > xb) continue;
                    const int rowbase = (z * g.ny + y) * g.nx;
                    const int pbeg = st[rowbase + xa], pend = st[rowbase + xb + 1];
                    int p = pbeg;
                    for (; p + 4 <= pend; p += 4) {          // four candidate loads in flight
                        const float4 s0 = sorted[p], s1 = sorted[p + 1], s2 = sorted[p + 2], s3 = sorted[p + 3];
                        consider(s0); consider(s1); consider(s2); consider(s3);
                    }
                    for (; p < pend; ++p) consider(sorted[p]);
                }
            }
        }
        flush();
        // every point outside the cube of rings <= r is at least `gap` away along some axis
        float gap = 3.4e38f;
        if (c.x - r > 0) gap = fminf(gap, qx - (g.ox + (float)(c.x - r) * g.cell));
        if (c.x + r + 1 < g.nx) gap = fminf(gap, (g.ox + (float)(c.x + r + 1) * g.cell) - qx);
        if (c.y - r > 0) gap = fminf(gap, qy - (g.oy + (float)(c.y - r) * g.cell));
        if (c.y + r + 1 < g.ny) gap = fminf(gap, (g.oy + (float)(c.y + r + 1) * g.cell) - qy);
        if (c.z - r > 0) gap = fminf(gap, qz - (g.oz + (float)(c.z - r) * g.cell));
        if (c.z + r + 1 < g.nz) gap = fminf(gap, (g.oz + (float)(c.z + r + 1) * g.cell) - qz);
        if (gap >= 3.0e38f) break;  // the cube covers the whole grid
        const float safe = gap - g.margin;
        if (safe > 0.f && best.kth() < safe * safe) break;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k >= KM - K) {
            int id = (int)(unsigned int)(best.key[k] & 0xffffffffull) + id0;
            if constexpr (Split::RAGGED) { if (best.key[k] == KNN_KEY_INF) id = -1; }      // the cloud ran out of points (or the distance is NaN)
            if (out64) out64[o + k - (KM - K)] = id;
            if (out32) out32[o + k - (KM - K)] = id;
        }
    }
}

// ------------------------------------------------------------------ 5b. query, sixteen lanes per query (K <= 16)
// The one-lane search above is a chain of ~100 dependent round trips per query (cell start -> candidates, segment by
// segment).  Here the row segments of a ring are dealt over the SIXTEEN lanes of a query group (four queries per
// wavefront): ring 1 = the 3 x 3 x 3 cube as nine x-rows, ring r >= 2 = the shell's 8r face rows (full x-span, one
// contiguous candidate range each) plus two end cells for each of its (2r - 1)^2 inner rows.  (A first round of the
// nine centre rows FIVE cells wide, so that cube 2 needs only its sixteen face rows afterwards, measured slower -- 371
// against 233 us: indoor clouds are surfaces, an occupied cell holds several points, and the rank selection is quadratic
// in the candidates that arrive before a bound exists.)  Accepted keys
// (key < bound) are appended to a per-query LDS pool (LDS atomic slot counter); after every ring -- and whenever the
// pool could overflow -- the group ranks the pool entries against each other (entry i's rank = number of smaller keys)
// and the sixteen smallest land, sorted, in slots 0..15: that is the running top-K, its last key the new bound, and
// at the end the output row.  Same keys, same stop test -> same tables as the one-lane kernel.
#ifndef CO_LPQ_
#define CO_LPQ_ 16          // lanes per query; swept on 4 x 40960 self-queries: 8 lanes 262 us, 16 lanes 232 us, 32 lanes 289 us per call
#endif
#ifndef CO_CAP_
#define CO_CAP_ 128
#endif
constexpr int CO_LPQ = CO_LPQ_, CO_BLOCK = 256, CO_QPB = CO_BLOCK / CO_LPQ, CO_CAP = CO_CAP_, CO_CHUNK = 4;
constexpr int CO_ROUND = CO_LPQ * CO_CHUNK;          // appends of one chunk round at most

template <int KM, class Split>      // K <= KM <= 16
__global__ __launch_bounds__(CO_BLOCK) void knn_coop_kernel(const float* __restrict__ queries, const Split split, int K,
                                                            const GridInfo* __restrict__ info,
                                                            const int32_t* __restrict__ starts,
                                                            const float4* __restrict__ sorted,
                                                            int64_t* __restrict__ out64, int32_t* __restrict__ out32) {
    static_assert(KM <= 16, "the running top-K lives in pool slots 0..15");
    __shared__ unsigned long long s_pool[2][CO_QPB][CO_CAP];       // double-buffered: a compaction writes the other buffer
    __shared__ int s_cnt[CO_QPB];
    const int l = threadIdx.x & (CO_LPQ - 1), qs = threadIdx.x / CO_LPQ;
    const int gshift = (threadIdx.x & 63) & ~(CO_LPQ - 1);         // first lane of this group inside its wavefront
    int64_t qi = (int64_t)blockIdx.x * CO_QPB + qs;
    const bool qvalid = qi < split.queries_x();
    if (!qvalid) qi = split.queries_x() - 1;
    const Row row = split.query(qi);                               // ragged: not live = a query of no segment; it searches nothing (rmax)
    const int b = row.b;
    const GridInfo g = info[b];
    const float* qp = queries + row.row * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const int3 c = cell_of<Split::RAGGED>(g, qx, qy, qz);
    const int32_t* st = starts + split.cell0(b);
    unsigned long long* pool = s_pool[0][qs];
    int which = 0;
    if (l == 0) s_cnt[qs] = 0;
    __builtin_amdgcn_wave_barrier();
    unsigned long long bound = KNN_KEY_INF;

    // rank selection: slots 0..min(n, 16)-1 of the OTHER buffer <- the smallest keys in ascending order
    auto compact = [&]() {
        __builtin_amdgcn_wave_barrier();
        const int n = s_cnt[qs];
        unsigned long long* dst = s_pool[which ^ 1][qs];
        for (int i = l; i < n; i += CO_LPQ) {                    // this lane's entries, one after the other
            const unsigned long long mine = pool[i];
            int rank = 0;
            int j = 0;
            for (; j + 4 <= n; j += 4) {                         // one address per group and read: LDS broadcasts
                const unsigned long long p0 = pool[j], p1 = pool[j + 1], p2 = pool[j + 2], p3 = pool[j + 3];
                rank += (p0 < mine ? 1 : 0) + (p1 < mine ? 1 : 0) + (p2 < mine ? 1 : 0) + (p3 < mine ? 1 : 0);
            }
            for (; j < n; ++j) rank += pool[j] < mine ? 1 : 0;
            if (rank < 16) dst[rank] = mine;
        }
        const int m = n < 16 ? n : 16;
        if (l == 0) s_cnt[qs] = m;
        which ^= 1;
        pool = dst;
        __builtin_amdgcn_wave_barrier();
        bound = m >= K ? pool[K - 1] : KNN_KEY_INF;
    };
    // this lane's candidate range [pb, pe) of the ring's slot `s`; empty when the slot lies outside the grid
    auto segment = [&](int r, int s, int& pb, int& pe) {
        pb = pe = 0;
        int dz, dy, xa, xb;
        const int side = 2 * r + 1;
        if (r == 1) {
            if (s >= 9) return;
            dz = s / 3 - 1; dy = s % 3 - 1; xa = c.x - 1; xb = c.x + 1;
        } else {
            const int nface = 8 * r, inner = side - 2;
            if (s < nface) {
                if (s < side) { dz = -r; dy = s - r; }
                else if (s < 2 * side) { dz = r; dy = s - side - r; }
                else { const int k = s - 2 * side; dz = (k >> 1) - r + 1; dy = (k & 1) ? r : -r; }
                xa = c.x - r; xb = c.x + r;
            } else {
                const int k = s - nface;
                if (k >= 2 * inner * inner) return;
                const int row = k >> 1;
                const int rq = (int)(((float)row + 0.5f) / (float)inner);      // row / inner (the margin 0.5 / inner >> float error)
                dz = rq - r + 1; dy = row - rq * inner - r + 1;
                xa = xb = (k & 1) ? c.x + r : c.x - r;
                if (xa < 0 || xa >= g.nx) return;
            }
        }
        const int z = c.z + dz, y = c.y + dy;
        if (z < 0 || z >= g.nz || y < 0 || y >= g.ny) return;
        xa = max(xa, 0); xb = min(xb, g.nx - 1);
        if (xa > xb) return;
        const int rowbase = (z * g.ny + y) * g.nx;
        pb = st[rowbase + xa];
        pe = st[rowbase + xb + 1];
    };
    // Termination: r and the slots s0 run over the grid's extent (n <= 161 per axis), and every pass of the for (;;) below moves
    // each lane's pb forward by CO_CHUNK towards a pe inside the cloud's part of `sorted` -- no bound depends on how many
    // neighbours were found or on the query's coordinates.  A cloud with fewer than K points (the ragged form) keeps `bound`
    // infinite, the stop test at the end of the ring never holds, and the search ends at the ring whose cube covers the grid; a
    // NaN / infinite query makes the gap comparisons false or the gap infinite and ends no later.
    const int rmax = !Split::RAGGED || row.live ? max(g.nx, max(g.ny, g.nz)) : 0;
    int room = CO_CAP;                                  // free pool slots, counted conservatively (group-uniform)
    for (int r = 1; r <= rmax; ++r) {
        const int side = 2 * r + 1;
        const int nslot = r == 1 ? 9 : 8 * r + 2 * (side - 2) * (side - 2);
        for (int s0 = 0; s0 < nslot; s0 += CO_LPQ) {
            int pb, pe;
            segment(r, s0 + l, pb, pe);
            for (;;) {
                const unsigned long long vote = __ballot(pb < pe);
                if (((vote >> gshift) & ((1ull << CO_LPQ) - 1ull)) == 0ull) break;
                if (room < CO_ROUND) {                              // the conservative count says the pool could overflow
                    __builtin_amdgcn_wave_barrier();
                    room = CO_CAP - s_cnt[qs];
                    if (room < CO_ROUND) {
                        compact();
                        room = CO_CAP - 16;
                    }
                }
                if (bound == KNN_KEY_INF && CO_CAP - room >= K) {
                    // no exact K-th key yet (fewer than K candidates at the last compaction), but the pool may hold K
                    // entries by now: the largest of ANY K candidates is an upper bound of the K-th smallest
                    __builtin_amdgcn_wave_barrier();
                    if (s_cnt[qs] >= K) {
                        unsigned long long v = 0ull;
                        for (int i = l; i < K; i += CO_LPQ) v = pool[i] > v ? pool[i] : v;
#pragma unroll
                        for (int o = 1; o < CO_LPQ; o <<= 1) {
                            const unsigned long long w = __shfl_xor(v, o, WAVE);
                            v = w > v ? w : v;
                        }
                        bound = v + 1ull;                           // the entry itself stays eligible (it is in the pool already)
                    }
                }
                float4 cand[CO_CHUNK];
#pragma unroll
                for (int u = 0; u < CO_CHUNK; ++u) cand[u] = sorted[pb + u < pe ? pb + u : (pb < pe ? pb : 0)];
                unsigned long long key[CO_CHUNK];
                bool ok[CO_CHUNK];
                int k = 0;
#pragma unroll
                for (int u = 0; u < CO_CHUNK; ++u) {
                    key[u] = knn_key(sqdist_exact(qx, qy, qz, cand[u].x, cand[u].y, cand[u].z), __float_as_int(cand[u].w));
                    ok[u] = pb + u < pe && key[u] < bound;
                    k += ok[u] ? 1 : 0;
                }
                if (k > 0) {                                        // one slot reservation per lane and round
                    int slot = atomicAdd(&s_cnt[qs], k);
#pragma unroll
                    for (int u = 0; u < CO_CHUNK; ++u)
                        if (ok[u]) pool[slot++] = key[u];
                }
                room -= CO_ROUND;
                pb += CO_CHUNK;
            }
        }
        compact();
        room = CO_CAP - 16;
        float gap = 3.4e38f;                // as the one-lane kernel: distance to the nearest face of the searched cube
        if (c.x - r > 0) gap = fminf(gap, qx - (g.ox + (float)(c.x - r) * g.cell));
        if (c.x + r + 1 < g.nx) gap = fminf(gap, (g.ox + (float)(c.x + r + 1) * g.cell) - qx);
        if (c.y - r > 0) gap = fminf(gap, qy - (g.oy + (float)(c.y - r) * g.cell));
        if (c.y + r + 1 < g.ny) gap = fminf(gap, (g.oy + (float)(c.y + r + 1) * g.cell) - qy);
        if (c.z - r > 0) gap = fminf(gap, qz - (g.oz + (float)(c.z - r) * g.cell));
        if (c.z + r + 1 < g.nz) gap = fminf(gap, (g.oz + (float)(c.z + r + 1) * g.cell) - qz);
        if (gap >= 3.0e38f) break;
        const float safe = gap - g.margin;
        const float kth = __uint_as_float((unsigned int)(bound >> 32));
        if (safe > 0.f && bound != KNN_KEY_INF && kth < safe * safe) break;
    }
    if (qvalid) {
        const int id0 = split.id0(b);
        int found = K;
        if constexpr (Split::RAGGED) found = s_cnt[qs];            // pool entries after the last compaction; fewer than K: the cloud ran out
        for (int i = l; i < K; i += CO_LPQ) {
            const int id = i < found ? (int)(unsigned int)(pool[i] & 0xffffffffull) + id0 : -1;
            const int64_t o = row.row * K + i;
            if (out64) out64[o] = id;
            if (out32) out32[o] = id;
        }
    }
}

// ------------------------------------------------------------------ small clouds: no grid, sixteen lanes per query
// The grid search above is ONE lane per query walking ~100 dependent (cell start -> candidates) round trips: its time
// barely depends on the number of queries (213 us for 4 x 40960 self-queries, still 123 us for 4 x 320), so the coarse
// levels of the collate cost as much as the fine ones.  For clouds of <= BRUTE_MAX points every query instead looks at
// EVERY point of its cloud, sixteen lanes per query: lane l ranks candidates l, l + 16, ... (same 64-bit (distance, id)
// keys, same parked-insert queue), starting at the query's own neighbourhood in memory order -- the collate keeps every
// level Morton-sorted, so the first window already gives a tight bound -- then the sixteen sorted lists are merged by
// K rounds of group-wide minimum.  No grid construction (seven launches less per call), results identical: the K smallest
// keys of a set do not depend on the order they are offered in.
constexpr int BRUTE_MAX = 4096, BRUTE_LPQ = 16, BRUTE_BLOCK = 256, BRUTE_QPB = BRUTE_BLOCK / BRUTE_LPQ;
constexpr Widths<1, 8, 16, 32> KNN_BRUTE_KS{};      // the K the whole-cloud search is compiled for (K == KM exactly)

__device__ __forceinline__ unsigned long long group16_min(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < BRUTE_LPQ; o <<= 1) {
        const unsigned long long w = __shfl_xor(v, o, WAVE);
        v = w < v ? w : v;
    }
    return v;
}

template <int KM>      // K == KM exactly
__global__ __launch_bounds__(BRUTE_BLOCK) void knn_brute_kernel(const float* __restrict__ pts, int64_t npts,
                                                                const float* __restrict__ queries, int64_t nq,
                                                                int64_t* __restrict__ out64, int32_t* __restrict__ out32) {
    constexpr bool QUEUED = KM > 1;
    __shared__ unsigned long long s_queue[QUEUED ? QCAP * BRUTE_BLOCK : 1];
    const int b = blockIdx.y;
    const int l = threadIdx.x & (BRUTE_LPQ - 1);
    int64_t qi = (int64_t)blockIdx.x * BRUTE_QPB + (threadIdx.x >> 4);
    const bool qvalid = qi < nq;
    if (!qvalid) qi = nq - 1;                              // keep every lane in the wave-wide votes and shuffles
    const float* qp = queries + ((int64_t)b * nq + qi) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float* P = pts + (int64_t)b * npts * 3;
    const int n = (int)npts;
    // scan order: start 32 points before the query's proportional position in the candidate array, wrap around
    int start = ((int)((qi * npts) / nq) - 32) % n;
    if (start < 0) start += n;

    TopK<KM> best;
    best.init(KM);
    int cnt = 0;
    unsigned long long bound = KNN_KEY_INF;
    auto flush = [&]() {
        if constexpr (QUEUED) {
            for (int i = 0; i < QCAP; ++i) {
                if (!__any(i < cnt)) break;
                if (i < cnt) best.offer(s_queue[i * BRUTE_BLOCK + threadIdx.x]);
            }
            cnt = 0;
            // every lane of the group may use the smallest K-th key among the sixteen lists: that list alone already
            // holds K candidates at or below it
            bound = group16_min(best.kth_key());
        }
    };
    auto consider = [&](float px, float py, float pz, int id, bool live) {
        const unsigned long long key = knn_key(sqdist_exact(qx, qy, qz, px, py, pz), id);
        if constexpr (QUEUED) {
            if (live && key < bound) {
                s_queue[cnt * BRUTE_BLOCK + threadIdx.x] = key;
                ++cnt;
            }
            if (__any(cnt == QCAP)) flush();
        } else {
            if (live) best.offer(key);
        }
    };
    const int rounds = (n + BRUTE_LPQ - 1) / BRUTE_LPQ;
    int t = 0;
    for (; t + 4 <= rounds; t += 4) {                      // four candidates per lane in flight
        int id[4];
        float c[4][3];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = (t + u) * BRUTE_LPQ + l;
            live[u] = i < n;
            int j = start + (live[u] ? i : 0);
            if (j >= n) j -= n;
            id[u] = j;
            c[u][0] = P[3 * j]; c[u][1] = P[3 * j + 1]; c[u][2] = P[3 * j + 2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) consider(c[u][0], c[u][1], c[u][2], id[u], live[u]);
        if (t == 0) flush();                               // the first window fixes a tight bound early
    }
    for (; t < rounds; ++t) {
        const int i = t * BRUTE_LPQ + l;
        const bool live = i < n;
        int j = start + (live ? i : 0);
        if (j >= n) j -= n;
        consider(P[3 * j], P[3 * j + 1], P[3 * j + 2], j, live);
    }
    flush();
    // merge: K rounds, each takes the smallest head of the sixteen lists; the owning lane drops it
    const int64_t o = ((int64_t)b * nq + qi) * KM;
#pragma unroll 1
    for (int k = 0; k < KM; ++k) {
        const unsigned long long mine = best.key[0];
        const unsigned long long mn = group16_min(mine);
        if (mine == mn) {                                  // keys are unique (ids are): exactly one lane
#pragma unroll
            for (int i = 0; i + 1 < KM; ++i) best.key[i] = best.key[i + 1];
            best.key[KM - 1] = KNN_KEY_INF;
        }
        if (l == 0 && qvalid) {
            const int id = (int)(unsigned int)(mn & 0xffffffffull);
            if (out64) out64[o + k] = id;
            if (out32) out32[o + k] = id;
        }
    }
}

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

static double knn_points_per_cell() { return 0.6; }      // sweep 0.35 .. 16 on the bench clouds: flat optimum around 0.6

static int grid_g0(size_t npts) {
    int g = (int)floor(cbrt((double)npts / knn_points_per_cell()));
    if (g < 1) g = 1;
    if (g > 160) g = 160;
    return g;
}

struct KnnLayout {
    int G0, ncell_alloc;
    size_t off_info, off_cellid, off_counts, off_starts, off_fill, off_sorted, off_temp, temp_bytes, total;
};

static KnnLayout knn_layout(size_t B, size_t npts) {
    KnnLayout L;
    L.G0 = grid_g0(npts);
    L.ncell_alloc = (L.G0 + 1) * (L.G0 + 1) * (L.G0 + 1);
    const size_t ncell_total = B * (size_t)L.ncell_alloc + 1;
    size_t o = 0;
    L.off_info = o;   o += al(sizeof(GridInfo) * B);
    L.off_cellid = o; o += al(sizeof(int32_t) * B * npts);
    L.off_counts = o; o += al(sizeof(int32_t) * ncell_total);
    L.off_fill = o;   o += al(sizeof(int32_t) * ncell_total);   // counts and fill are zeroed together
    L.off_starts = o; o += al(sizeof(int32_t) * ncell_total);
    L.off_sorted = o; o += al(sizeof(float4) * B * npts);
    const size_t tb = sizeof(int32_t) * scan_block_sums((int64_t)ncell_total);
    L.temp_bytes = tb;
    L.off_temp = o;   o += al(tb);
    L.total = o + 256;
    return L;
}

// ---- the ragged form's workspace.  The split reaches the device only, so the cell arrays are sized by a bound over ALL splits:
//
//   cells(split) = sum_s seg_cells(n_s) <= 8 S + 4 N        for S segments with sum_s n_s <= N.
//
// Proof, segment by segment: seg_cells(n) = (g + 1)^3 with g = seg_g0(n).  g = 1: 8 cells.  g >= 2 needs 3 g^3 <= 5 n, i.e.
// n >= 0.6 g^3, and (g + 1)^3 <= 8 + 2.4 g^3 <= 8 + 4 n: for g = 2, 27 <= 27.2; for g >= 3, (1 + 1/g)^3 <= (4/3)^3 < 2.4 (the cap
// g <= 160 only lowers the left side).  So seg_cells(n) <= 8 + 4 n for every n >= 0, and the sum over the segments is the claim.
// sum n_s <= N holds for ANY pointer array, because segments_kernel turns it into ascending boundaries inside [0, N].
// (A single cloud needs about N / 0.6 cells: the bound costs 2.4 times that, 48 bytes per point over the three cell arrays.)
// tests/test_host_knn_segments.py checks the bound against crfconv_knn_segments_need on random and extreme splits.
static size_t seg_cells_bound(size_t S, size_t N) { return 8 * S + 4 * N; }

struct SegLayout {
    size_t ncell_total, off_info, off_pb, off_qb, off_cb, off_cellid, off_counts, off_starts, off_fill, off_sorted, off_temp, total;
};

static SegLayout seg_layout(size_t S, size_t N, size_t cells) {
    SegLayout L;
    L.ncell_total = cells + 1;                  // + 1: the last cloud's searches read the start one past its last cell
    size_t o = 0;
    L.off_info = o;   o += al(sizeof(GridInfo) * S);
    L.off_pb = o;     o += al(sizeof(int32_t) * (S + 1));
    L.off_qb = o;     o += al(sizeof(int32_t) * (S + 1));
    L.off_cb = o;     o += al(sizeof(int32_t) * (S + 1));
    L.off_cellid = o; o += al(sizeof(int32_t) * N);
    L.off_counts = o; o += al(sizeof(int32_t) * L.ncell_total);
    L.off_fill = o;   o += al(sizeof(int32_t) * L.ncell_total);   // counts and fill are zeroed together
    L.off_starts = o; o += al(sizeof(int32_t) * L.ncell_total);
    L.off_sorted = o; o += al(sizeof(float4) * N);
    L.off_temp = o;   o += al(sizeof(int32_t) * scan_block_sums((int64_t)L.ncell_total));
    L.total = o + 256;
    return L;
}

struct GridArrays {        // the grid's arrays inside a workspace (KnnLayout or SegLayout)
    GridInfo* info;
    int32_t *cell_id, *counts, *fill, *starts, *temp;
    float4* sorted;
    size_t ncell_total, zero16;         // cells to scan; 16-byte words of counts + fill
};

// zero | bbox | histogram | scan | scatter | search: the launches of both entries.  px / qx = point / query rows along blockIdx.x,
// ny = gridDim.y (the clouds of a UniformSplit; 1 for a RaggedSplit, whose rows find their segment themselves).
template <class Split>
static int grid_knn(const Split& split, const GridArrays& A, const float* pts, size_t n_clouds, size_t px, size_t ny, const float* queries,
                    size_t qx, size_t K, int64_t* out_i64, int32_t* out_i32, hipStream_t st) {
    // counts + fill.  A kernel, not hipMemsetAsync: captured into a hipGraph, the memset NODE of this call faulted ("Memory
    // access fault ... write access to a read-only page") as soon as any eager launch ran between two replays (ROCm 7.2,
    // scratch/cg_diag2.py), while kernel nodes replay fine.
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)std::min<size_t>(1024, (A.zero16 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(A.counts), A.zero16);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(bbox_kernel<Split>, dim3((unsigned)n_clouds), dim3(1024), 0, st, pts, split, A.info);
    CRF_LAUNCH_CHECK();
    const dim3 pgrid((unsigned)cdiv((int64_t)px, 256), (unsigned)ny);
    if (px > 0) {
        hipLaunchKernelGGL(cell_count_kernel<Split>, pgrid, dim3(256), 0, st, pts, split, A.info, A.cell_id, A.counts);
        CRF_LAUNCH_CHECK();
    }
    exclusive_scan_i32(A.counts, A.starts, (int64_t)A.ncell_total, A.temp, st);
    if (px > 0) {
        hipLaunchKernelGGL(cell_scatter_kernel<Split>, pgrid, dim3(256), 0, st, pts, split, A.cell_id, A.starts, A.fill, A.sorted);
        CRF_LAUNCH_CHECK();
    }
    if (K > 1 && K <= 16) {
        const dim3 cgrid((unsigned)cdiv((int64_t)qx, CO_QPB), (unsigned)ny);
        hipLaunchKernelGGL((knn_coop_kernel<16, Split>), cgrid, dim3(CO_BLOCK), 0, st, queries, split, (int)K, A.info, A.starts, A.sorted,
                           out_i64, out_i32);
        CRF_LAUNCH_CHECK();
        return CRF_OK;
    }
    const dim3 qgrid((unsigned)cdiv((int64_t)qx, QBLOCK), (unsigned)ny);
    dispatch_width(KNN_QUERY_CAPS, K == 1 ? 1 : K <= 32 ? 32 : 64, [&](auto KM) {
        hipLaunchKernelGGL((knn_query_kernel<decltype(KM)::value, Split>), qgrid, dim3(QBLOCK), 0, st, queries, split, (int)K, A.info,
                           A.starts, A.sorted, out_i64, out_i32);
    });
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_knn_batch_dev_workspace(size_t batch_size, size_t npts, size_t nqueries, size_t K) {
    (void)nqueries; (void)K;
    if (batch_size == 0 || npts == 0) return 0;
    return knn_layout(batch_size, npts).total;
}

extern "C" int crfconv_knn_batch_dev(const float* pts, size_t batch_size, size_t npts, size_t dim,
                                     const float* queries, size_t nqueries, size_t K, int64_t* out_i64,
                                     int32_t* out_i32, void* workspace, size_t workspace_bytes,
                                     crf_stream_t stream) {
    CRF_REQUIRE(pts && queries && workspace && (out_i64 || out_i32), CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(dim == 3, CRF_ERR_UNSUPPORTED, "kNN supports dim == 3 only (got %zu)", dim);
    CRF_REQUIRE(batch_size >= 1 && batch_size <= 65535 && npts >= 1 && nqueries >= 1, CRF_ERR_ARG, "empty input");
    CRF_REQUIRE(K >= 1 && K <= 64 && K <= npts, CRF_ERR_ARG, "K=%zu must satisfy 1 <= K <= min(64, npts=%zu)", K, npts);
    CRF_REQUIRE(batch_size * npts < ((size_t)1 << 31), CRF_ERR_UNSUPPORTED, "B*npts too large");
    const KnnLayout L = knn_layout(batch_size, npts);
    CRF_REQUIRE(workspace_bytes >= L.total, CRF_ERR_WORKSPACE, "knn workspace %zu < %zu", workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    // Which search serves which (npts, K):
    //   npts <= BRUTE_MAX and K in KNN_BRUTE_KS   the whole-cloud search, no grid;
    //   otherwise the grid, searched by           1 < K <= 16: sixteen lanes per query;
    //                                             K == 1, K > 16: one lane per query, capacity 1, 32 or 64.
    if (npts <= (size_t)BRUTE_MAX) {
        const dim3 bgrid((unsigned)cdiv((int64_t)nqueries, BRUTE_QPB), (unsigned)batch_size);
        const bool whole = dispatch_width(KNN_BRUTE_KS, (int)K, [&](auto KM) {
            hipLaunchKernelGGL(knn_brute_kernel<decltype(KM)::value>, bgrid, dim3(BRUTE_BLOCK), 0, st, pts, (int64_t)npts, queries,
                               (int64_t)nqueries, out_i64, out_i32);
        });
        if (whole) {
            CRF_LAUNCH_CHECK();
            return CRF_OK;
        }
    }
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    GridArrays A;
    A.info = reinterpret_cast<GridInfo*>(ws + L.off_info);
    A.cell_id = reinterpret_cast<int32_t*>(ws + L.off_cellid);
    A.counts = reinterpret_cast<int32_t*>(ws + L.off_counts);
    A.fill = reinterpret_cast<int32_t*>(ws + L.off_fill);
    A.starts = reinterpret_cast<int32_t*>(ws + L.off_starts);
    A.sorted = reinterpret_cast<float4*>(ws + L.off_sorted);
    A.temp = reinterpret_cast<int32_t*>(ws + L.off_temp);
    A.ncell_total = batch_size * (size_t)L.ncell_alloc + 1;
    A.zero16 = (L.off_starts - L.off_counts) / 16;                       // the regions are 256-byte aligned
    const UniformSplit split{(int64_t)npts, (int64_t)nqueries, L.ncell_alloc, L.G0};
    return grid_knn(split, A, pts, batch_size, npts, batch_size, queries, nqueries, K, out_i64, out_i32, st);
}

extern "C" size_t crfconv_knn_segments_dev_workspace(size_t n_segments, size_t total_pts, size_t total_queries, size_t K) {
    (void)total_queries; (void)K;
    if (n_segments == 0) return 0;
    return seg_layout(n_segments, total_pts, seg_cells_bound(n_segments, total_pts)).total;
}

extern "C" size_t crfconv_knn_segments_need(const int64_t* seg_sizes, size_t n_segments) {
    size_t N = 0, cells = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        const int64_t n = seg_sizes[s] > 0 ? seg_sizes[s] : 0;
        N += (size_t)n;
        cells += (size_t)seg_cells(n);
    }
    return n_segments ? seg_layout(n_segments, N, cells).total : 0;
}

extern "C" int crfconv_knn_segments_dev(const float* pts, const int64_t* pts_ptr, const float* queries, const int64_t* q_ptr,
                                        size_t n_segments, size_t total_pts, size_t total_queries, size_t dim, size_t K,
                                        int64_t* out_i64, int32_t* out_i32, void* workspace, size_t workspace_bytes,
                                        crf_stream_t stream) {
    CRF_REQUIRE(pts_ptr && q_ptr && workspace && (out_i64 || out_i32) && (pts || !total_pts) && (queries || !total_queries), CRF_ERR_ARG,
                "null pointer");
    CRF_REQUIRE(dim == 3, CRF_ERR_UNSUPPORTED, "kNN supports dim == 3 only (got %zu)", dim);
    CRF_REQUIRE(n_segments >= 1 && n_segments <= 65535, CRF_ERR_ARG, "n_segments=%zu must satisfy 1 <= n_segments <= 65535", n_segments);
    CRF_REQUIRE(K >= 1 && K <= 64, CRF_ERR_ARG, "K=%zu must satisfy 1 <= K <= 64", K);
    CRF_REQUIRE(total_pts < ((size_t)1 << 31) && seg_cells_bound(n_segments, total_pts) + 1 < ((size_t)1 << 31), CRF_ERR_UNSUPPORTED,
                "total_pts=%zu too large (cell positions are int32)", total_pts);
    CRF_REQUIRE(total_queries < ((size_t)1 << 28), CRF_ERR_UNSUPPORTED, "total_queries=%zu too large for one launch", total_queries);
    const SegLayout L = seg_layout(n_segments, total_pts, seg_cells_bound(n_segments, total_pts));
    CRF_REQUIRE(workspace_bytes >= L.total, CRF_ERR_WORKSPACE, "knn workspace %zu < %zu", workspace_bytes, L.total);
    if (total_queries == 0) return CRF_OK;
    hipStream_t st = as_stream(stream);
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    GridArrays A;
    A.info = reinterpret_cast<GridInfo*>(ws + L.off_info);
    A.cell_id = reinterpret_cast<int32_t*>(ws + L.off_cellid);
    A.counts = reinterpret_cast<int32_t*>(ws + L.off_counts);
    A.fill = reinterpret_cast<int32_t*>(ws + L.off_fill);
    A.starts = reinterpret_cast<int32_t*>(ws + L.off_starts);
    A.sorted = reinterpret_cast<float4*>(ws + L.off_sorted);
    A.temp = reinterpret_cast<int32_t*>(ws + L.off_temp);
    A.ncell_total = L.ncell_total;
    A.zero16 = (L.off_starts - L.off_counts) / 16;
    int32_t* pb = reinterpret_cast<int32_t*>(ws + L.off_pb);
    int32_t* qb = reinterpret_cast<int32_t*>(ws + L.off_qb);
    int32_t* cb = reinterpret_cast<int32_t*>(ws + L.off_cb);
    hipLaunchKernelGGL(segments_kernel, dim3(1), dim3(SEG_BLOCK), 0, st, pts_ptr, q_ptr, (int)n_segments, (int)total_pts, (int)total_queries,
                       pb, qb, cb);
    CRF_LAUNCH_CHECK();
    const RaggedSplit split{pb, qb, cb, (int)n_segments, (int)total_pts, (int)total_queries};
    return grid_knn(split, A, pts, n_segments, total_pts, 1, queries, total_queries, K, out_i64, out_i32, st);
}

// ------------------------------------------------------------------ host-buffer forms (knn_.h signatures)
static int knn_host(const float* pts, size_t B, size_t npts, size_t dim, const float* queries, size_t nq,
                    size_t K, long* out) {
    CRF_REQUIRE(pts && queries && out, CRF_ERR_ARG, "null pointer");
    CRF_REQUIRE(dim == 3, CRF_ERR_UNSUPPORTED, "kNN supports dim == 3 only (got %zu)", dim);
    const size_t wsb = crfconv_knn_batch_dev_workspace(B, npts, nq, K);
    float *dp = nullptr, *dq = nullptr;
    int64_t* dout = nullptr;
    void* ws = nullptr;
    int rc = CRF_OK;
    hipError_t e;
#define TRY(x) if ((e = (x)) != hipSuccess) { set_error("%s: %s", #x, hipGetErrorString(e)); rc = CRF_ERR_HIP; goto done; }
    TRY(hipMalloc(&dp, sizeof(float) * 3 * B * npts));
    TRY(hipMalloc(&dq, sizeof(float) * 3 * B * nq));
    TRY(hipMalloc(&dout, sizeof(int64_t) * B * nq * K));
    TRY(hipMalloc(&ws, wsb));
    TRY(hipMemcpy(dp, pts, sizeof(float) * 3 * B * npts, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dq, queries, sizeof(float) * 3 * B * nq, hipMemcpyHostToDevice));
    rc = crfconv_knn_batch_dev(dp, B, npts, dim, dq, nq, K, dout, nullptr, ws, wsb, nullptr);
    if (rc != CRF_OK) goto done;
    TRY(hipStreamSynchronize(nullptr));
    static_assert(sizeof(long) == sizeof(int64_t), "LP64 expected");
    TRY(hipMemcpy(out, dout, sizeof(int64_t) * B * nq * K, hipMemcpyDeviceToHost));
#undef TRY
done:
    if (dp) (void)hipFree(dp);
    if (dq) (void)hipFree(dq);
    if (dout) (void)hipFree(dout);
    if (ws) (void)hipFree(ws);
    return rc;
}

extern "C" int crfconv_knn(const float* points, size_t npts, size_t dim, const float* queries,
                           size_t nqueries, size_t K, long* indices) {
    return knn_host(points, 1, npts, dim, queries, nqueries, K, indices);
}
extern "C" int crfconv_knn_omp(const float* points, size_t npts, size_t dim, const float* queries,
                               size_t nqueries, size_t K, long* indices) {
    return knn_host(points, 1, npts, dim, queries, nqueries, K, indices);
}
extern "C" int crfconv_knn_batch(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
                                 const float* queries, size_t nqueries, size_t K, long* batch_indices) {
    return knn_host(batch_data, batch_size, npts, dim, queries, nqueries, K, batch_indices);
}
extern "C" int crfconv_knn_batch_omp(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
                                     const float* queries, size_t nqueries, size_t K, long* batch_indices) {
    return knn_host(batch_data, batch_size, npts, dim, queries, nqueries, K, batch_indices);
}
