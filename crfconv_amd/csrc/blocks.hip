// Sliding XY blocks of the scenes of a ragged batch -- the process_raw_path bodies of the reference's block datasets
// (datasets/scannet_dataset.py:58-117, s3dis_dataset.py:119-171, semantic3d_dataset.py:107-157, npm3d_dataset.py:90-144): align a scene
// to its minimum corner, lay a grid of blocks every `stride`, give a block the points inside it plus a padding ring, drop blocks with too
// few points or too small a share of them in the un-padded core.  The reference makes one boolean mask over the whole scene per block;
// here a POINT finds its (few) blocks:
//
//   count   sb_bounds (ordered-int atomic min / max per scene: order-free) | sb_grid (block counts in double, the scenes' offsets into ONE
//           flat numbering of all grid cells) | sb_count (one thread per point: its cells, +1 on the cell's count and core count; integer
//           atomics, one per wavefront and distinct cell) | sb_decide (keep flag, kept count, totals) | two int32 scans (scan.hpp): the rank
//           of every kept cell = its block number, and the blocks' row offsets
//   -- the caller's ONE host read: blocks, rows --
//   emit    sb_recount (a point's memberships in KEPT cells) | scan = the point's first slot | sb_emit: (key = block, value = row | core
//           flag << 31) at its own slots, i.e. in point order | rsort_pairs_u64 over the bits the block number needs: stable, so a block's
//           rows ascend, with no atomics on the output side | sb_blocks (ptr, scene, cell per block) | sb_finish (the per-row outputs)
//
// Which blocks hold a point is decided by ONE function, axis_span, in all three point passes: per axis it walks a small over-estimate of
// the candidate block indices and tests each with the exact float32 bounds.  The bounds are formed in double in the reference's operation
// order -- i * stride, - padding, (+ block_size) + padding -- with no contraction into an fma, and rounded once to float32: what NumPy
// compares a float32 array against.  The float32 bounds ascend with i, so a point's blocks on an axis are a run i0 .. i0 + ni - 1 and its
// core blocks a run inside it.
#include "common.hpp"

#include "../../include/crfconv_blocks.h"
#include "radix_sort.hpp"
#include "segment_bounds.hpp"        // the status bits, sb_ord / sb_unord, sb_scene_of, sb_bounds_kernel

namespace crf {

using Spec = crf_sliding_blocks_spec;

__device__ __forceinline__ double sb_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// blocks along an axis of extent `limit` (a float32 value, taken to double), the reference's two expressions; -1: more than SB_AXIS_MAX.
// The cap is what lets sb_axis_span's candidate range be exact: a block's float32 bounds differ from the real ones by at most 2^-24 of
// their size, below 2^-24 (SB_AXIS_MAX + 2) stride < stride / 2 in units of the block index, while the range is widened by 2.
constexpr double SB_AXIS_MAX = 4194304.0;                  // 2^22 blocks along x or y
__device__ __forceinline__ int sb_axis_blocks(float limit, const Spec& sp) {
    const double d = dadd_rn((double)limit, -sp.block_size);
    const double q = sp.count_form == 0 ? ceil(sb_div(d, sp.stride)) : trunc(sb_div(ceil(d), sp.stride));      // int() truncates
    const double c = q + 1.0;
    if (!(c <= SB_AXIS_MAX)) return -1;                   // (NaN lands here too)
    return c < 0.0 ? 0 : (int)c;
}

// ONE workgroup: pos_min, limit, dims [S, 2] per scene, then cell_off [S + 1] -- the scenes' offsets in the flat cell numbering -- and
// totals: the cell count and the status
__global__ __launch_bounds__(256) void sb_grid_kernel(const unsigned* __restrict__ bnd, const int64_t* __restrict__ ptr, int S, Spec sp,
                                                      int64_t cell_cap, float* __restrict__ pos_min, float* __restrict__ limit,
                                                      int32_t* __restrict__ dims, int64_t* __restrict__ cell_off, int64_t* __restrict__ totals) {
    if (totals[SB_STATUS] != 0) return;
    __shared__ int s_over;
    if (threadIdx.x == 0) s_over = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) {
        int nx = 0, ny = 0;
        float mn[3] = {0.f, 0.f, 0.f}, lim[3] = {0.f, 0.f, 0.f};
        if (ptr[s + 1] > ptr[s]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mn[a] = sb_unord(bnd[6 * s + a]);
                lim[a] = sub_rn(-sb_unord(bnd[6 * s + 3 + a]), mn[a]);        // max(pos - min) = max(pos) - min: rounding is monotone
            }
            nx = sb_axis_blocks(lim[0], sp);
            ny = sb_axis_blocks(lim[1], sp);
            if (nx < 0 || ny < 0) { s_over = 1; nx = ny = 0; }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { pos_min[3 * s + a] = mn[a]; limit[3 * s + a] = lim[a]; }
        dims[2 * s] = nx;
        dims[2 * s + 1] = ny;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int64_t run = 0;
    bool over = s_over != 0;
    for (int s = 0; s < S; ++s) {
        cell_off[s] = run;
        run += (int64_t)dims[2 * s] * dims[2 * s + 1];
        if (run > 2147483647ll) { over = true; run = 0; }
    }
    cell_off[S] = run;
    totals[SB_CELLS] = run;
    totals[SB_STATUS] = over ? SB_OVERFLOW : (run > cell_cap ? SB_CELL_CAP : 0);
}

// A point's blocks along one axis: the run i0 .. i0 + ni - 1, and its core blocks c0 .. c0 + nc - 1 (inside the run).
struct Span { int i0, ni, c0, nc; };
__device__ __forceinline__ Span sb_axis_span(float x, int nb, const Spec& sp) {
    Span r = {0, 0, 0, 0};
    if (nb <= 0) return r;
    // i stride - padding <= x <= i stride + block_size + padding in exact arithmetic, widened by 2 either way: with at most SB_AXIS_MAX
    // blocks along the axis the float32 rounding of a bound moves it by less than half a stride (see SB_AXIS_MAX)
    const double xd = (double)x, top = (double)(nb - 1);
    double lo = floor((xd - sp.block_size - sp.padding) / sp.stride) - 2.0, hi = ceil((xd + sp.padding) / sp.stride) + 2.0;
    lo = lo < 0.0 ? 0.0 : lo;
    hi = hi > top ? top : hi;
    if (!(lo <= hi)) return r;
    const int ilo = (int)lo, ihi = (int)hi;
    for (int i = ilo; i <= ihi; ++i) {
        const double beg = dmul_rn((double)i, sp.stride), end = dadd_rn(beg, sp.block_size);
        const float pl = (float)dadd_rn(beg, -sp.padding), ph = (float)dadd_rn(end, sp.padding), cl = (float)beg, ch = (float)end;
        if (pl <= x && x <= ph) { if (r.ni == 0) r.i0 = i; ++r.ni; }
        if (cl <= x && x <= ch) { if (r.nc == 0) r.c0 = i; ++r.nc; }
    }
    return r;
}

// Everything a point pass needs: the point's runs on x and y, its scene's first cell and row length.  total = its memberships.
struct Member { Span x, y; int base, ny, total; };
__device__ __forceinline__ Member sb_member(const float* __restrict__ pos, const int64_t* __restrict__ ptr, int S, const Spec& sp,
                                            const float* __restrict__ pos_min, const int32_t* __restrict__ dims,
                                            const int64_t* __restrict__ cell_off, int64_t p) {
    const int s = sb_scene_of(ptr, S, p);
    Member m;
    m.x = sb_axis_span(sub_rn(pos[3 * p], pos_min[3 * s]), dims[2 * s], sp);
    m.y = sb_axis_span(sub_rn(pos[3 * p + 1], pos_min[3 * s + 1]), dims[2 * s + 1], sp);
    m.base = (int)cell_off[s];
    m.ny = dims[2 * s + 1];
    m.total = m.x.ni * m.y.ni;
    return m;
}
// membership t of a point, t < total (i-major, as the blocks are numbered): its cell, and whether the point is in the cell's core
__device__ __forceinline__ int sb_cell(const Member& m, int t, bool& core) {
    const int di = t / m.y.ni, i = m.x.i0 + di, j = m.y.i0 + (t - di * m.y.ni);
    core = i >= m.x.c0 && i < m.x.c0 + m.x.nc && j >= m.y.c0 && j < m.y.c0 + m.y.nc;
    return m.base + i * m.ny + j;
}

// One thread per point.  Round t handles every lane's t-th membership: the lanes of the wavefront that name the same cell find each
// other by ballot and ONE of them adds their number.  That merges adds only where neighbouring rows are neighbours in space (scan or
// Morton order); on rows in random order a wavefront names almost 64 different cells, nothing merges, and this launch is 88-92 % of the
// split's time (profiles/r33_sliding_blocks.md): contended same-address adds in L2.
__global__ __launch_bounds__(256) void sb_count_kernel(const float* __restrict__ pos, int64_t N, const int64_t* __restrict__ ptr, int S,
                                                       Spec sp, const float* __restrict__ pos_min, const int32_t* __restrict__ dims,
                                                       const int64_t* __restrict__ cell_off, const int64_t* __restrict__ totals,
                                                       int32_t* __restrict__ count, int32_t* __restrict__ core_count) {
    if (totals[SB_STATUS] != 0) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n_cells = (int)totals[SB_CELLS], lane = threadIdx.x & 63;
    Member m;
    m.total = 0;
    if (p < N) m = sb_member(pos, ptr, S, sp, pos_min, dims, cell_off, p);
    for (int t = 0;; ++t) {
        const bool act = t < m.total;
        unsigned long long rem = __ballot(act);
        if (rem == 0ull) break;                            // uniform
        bool core = false;
        int cell = -1;
        if (act) cell = sb_cell(m, t, core);
        while (rem != 0ull) {                              // uniform: one round per distinct cell
            const int leader = __ffsll((long long)rem) - 1;
            const int lc = __builtin_amdgcn_readlane(cell, leader);
            const unsigned long long same = __ballot(act && cell == lc), same_core = __ballot(act && cell == lc && core);
            if (lane == leader && lc >= 0 && lc < n_cells) {
                atomicAdd(&count[lc], __popcll(same));
                if (same_core != 0ull) atomicAdd(&core_count[lc], __popcll(same_core));
            }
            rem &= ~same;
        }
    }
}

// per cell (launched over the capacity; cells past the grid get zeros for the scans): kept?  totals += blocks, rows
__global__ __launch_bounds__(256) void sb_decide_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ core_count,
                                                        int64_t cell_cap, Spec sp, int64_t* __restrict__ totals,
                                                        int32_t* __restrict__ keep, int32_t* __restrict__ kept_count) {
    if (totals[SB_STATUS] != 0) return;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_cells = totals[SB_CELLS];
    int k = 0, n = 0;
    if (c < n_cells) {
        n = count[c];
        k = ((int64_t)n >= sp.min_points && sb_div((double)core_count[c], (double)n) >= sp.proportion) ? 1 : 0;    // 0 / 0: NaN, dropped
    }
    if (c < cell_cap) {
        keep[c] = k;
        kept_count[c] = k ? n : 0;
    }
    const unsigned long long kb = __ballot(k != 0);
    if (kb == 0ull) return;
    long long rows = k ? n : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o, WAVE);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&totals[SB_BLOCKS]), (unsigned long long)__popcll(kb));
        atomicAdd(reinterpret_cast<unsigned long long*>(&totals[SB_ROWS]), (unsigned long long)rows);
    }
}

__global__ __launch_bounds__(256) void sb_recount_kernel(const float* __restrict__ pos, int64_t N, const int64_t* __restrict__ ptr, int S,
                                                         Spec sp, const float* __restrict__ pos_min, const int32_t* __restrict__ dims,
                                                         const int64_t* __restrict__ cell_off, const int32_t* __restrict__ keep,
                                                         int32_t* __restrict__ point_rows) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const Member m = sb_member(pos, ptr, S, sp, pos_min, dims, cell_off, p);
    int n = 0;
    for (int t = 0; t < m.total; ++t) {
        bool core;
        n += keep[sb_cell(m, t, core)];
    }
    point_rows[p] = n;
}

__global__ __launch_bounds__(256) void sb_emit_kernel(const float* __restrict__ pos, int64_t N, const int64_t* __restrict__ ptr, int S,
                                                      Spec sp, const float* __restrict__ pos_min, const int32_t* __restrict__ dims,
                                                      const int64_t* __restrict__ cell_off, const int32_t* __restrict__ keep,
                                                      const int32_t* __restrict__ rank, const int32_t* __restrict__ point_slot,
                                                      int64_t n_rows, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const Member m = sb_member(pos, ptr, S, sp, pos_min, dims, cell_off, p);
    int64_t o = point_slot[p];
    for (int t = 0; t < m.total; ++t) {
        bool core;
        const int c = sb_cell(m, t, core);
        if (!keep[c]) continue;
        if (o < n_rows) {
            keys[o] = (unsigned long long)(unsigned)rank[c];
            vals[o] = (uint32_t)p | (core ? 0x80000000u : 0u);
        }
        ++o;
    }
}

// per kept cell: its block's row offset, scene and (i, j)
__global__ __launch_bounds__(256) void sb_blocks_kernel(const int32_t* __restrict__ keep, const int32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ row_off, const int32_t* __restrict__ dims,
                                                        const int64_t* __restrict__ cell_off, int S, int64_t n_blocks, int64_t n_rows,
                                                        int64_t* __restrict__ out_ptr, int64_t* __restrict__ scene, int32_t* __restrict__ cell) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c == 0) out_ptr[n_blocks] = n_rows;
    if (c >= cell_off[S] || !keep[c]) return;
    const int64_t b = rank[c];
    if (b >= n_blocks) return;
    const int s = sb_scene_of(cell_off, S, c);             // (a scene without cells repeats an entry, as an empty scene does in ptr)
    const int local = (int)(c - cell_off[s]), ny = dims[2 * s + 1];
    out_ptr[b] = row_off[c];
    scene[b] = s;
    cell[2 * b] = local / ny;
    cell[2 * b + 1] = local % ny;
}

__global__ __launch_bounds__(256) void sb_finish_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        int64_t n_rows, int64_t n_blocks, const int64_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ scene, int64_t* __restrict__ rows, int64_t* __restrict__ indices, int8_t* __restrict__ mask,
                                                        int64_t* __restrict__ batch) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t b = (int64_t)keys[r], row = (int64_t)(vals[r] & 0x7fffffffu);
    if (b >= n_blocks) return;                             // (cannot happen: every slot below n_rows was written by sb_emit)
    rows[r] = row;
    indices[r] = row - ptr[scene[b]];
    mask[r] = (int8_t)(vals[r] >> 31);
    batch[r] = b;
}

// minima and maxima of a block's aligned rows: one workgroup per block, order-free
__global__ __launch_bounds__(256) void sb_block_bounds_kernel(const float* __restrict__ pos, const float* __restrict__ pos_min,
                                                              const int64_t* __restrict__ rows, const int64_t* __restrict__ out_ptr,
                                                              const int64_t* __restrict__ scene, float* __restrict__ bounds) {
    __shared__ float s_v[4][6];
    const int64_t b = blockIdx.x, lo = out_ptr[b], hi = out_ptr[b + 1], s = scene[b];
    const float m0 = pos_min[3 * s], m1 = pos_min[3 * s + 1], m2 = pos_min[3 * s + 2];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) {
        const float* q = pos + 3 * rows[r];
        const float a0 = sub_rn(q[0], m0), a1 = sub_rn(q[1], m1), a2 = sub_rn(q[2], m2);
        v[0] = fminf(v[0], a0); v[1] = fminf(v[1], a1); v[2] = fminf(v[2], a2);
        v[3] = fmaxf(v[3], a0); v[4] = fmaxf(v[4], a1); v[5] = fmaxf(v[5], a2);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float u = __shfl_xor(v[k], o, WAVE);
            v[k] = k < 3 ? fminf(v[k], u) : fmaxf(v[k], u);
        }
        if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float u = s_v[0][k];
        for (int w = 1; w < 4; ++w) u = k < 3 ? fminf(u, s_v[w][k]) : fmaxf(u, s_v[w][k]);
        bounds[6 * b + k] = u;
    }
}

// one thread per row: pos_block = a, x = cat(extra, a / limit) (FORM 0) or cat(a - centre, extra) (FORM 1)
template <int FORM>
__global__ __launch_bounds__(256) void sb_features_kernel(const float* __restrict__ pos, const float* __restrict__ pos_min,
                                                          const float* __restrict__ limit, const float* __restrict__ extra, int F,
                                                          const int64_t* __restrict__ rows, const int64_t* __restrict__ batch,
                                                          const int64_t* __restrict__ scene, const float* __restrict__ bounds,
                                                          int64_t n_rows, float* __restrict__ pos_block, float* __restrict__ x) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t row = rows[r], b = batch[r], s = scene[b];
    float a[3], f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = sub_rn(pos[3 * row + k], pos_min[3 * s + k]);
    if constexpr (FORM == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = __fdiv_rn(a[k], limit[3 * s + k]);
    } else {
        const float* bb = bounds + 6 * b;
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = sub_rn(a[k], k == 2 ? bb[2] : __fdiv_rn(add_rn(bb[k], bb[3 + k]), 2.f));
    }
    float* xo = x + r * (3 + F);
    const float* e = extra + row * F;                      // (not read when F = 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pos_block[3 * r + k] = a[k];
        xo[(FORM == 0 ? F : 0) + k] = f[k];
    }
    for (int k = 0; k < F; ++k) xo[(FORM == 0 ? 0 : 3) + k] = e[k];
}

static size_t sb_al(size_t v) { return (v + 255) & ~(size_t)255; }

struct SbLayout { size_t bnd, dims, cell_off, count, core_count, keep, kept_count, rank, row_off, sums, total; };
static SbLayout sb_layout(int64_t S, int64_t cap) {
    SbLayout L;
    size_t o = 0;
    L.bnd = o;        o += sb_al(sizeof(unsigned) * 6 * (size_t)S);
    L.dims = o;       o += sb_al(sizeof(int32_t) * 2 * (size_t)S);
    L.cell_off = o;   o += sb_al(sizeof(int64_t) * ((size_t)S + 1));
    L.count = o;      o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.core_count = o; o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.keep = o;       o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.kept_count = o; o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.rank = o;       o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.row_off = o;    o += sb_al(sizeof(int32_t) * (size_t)cap);
    L.sums = o;       o += sb_al(sizeof(int32_t) * scan_block_sums(cap));
    L.total = o + 256;
    return L;
}

struct SbEmitLayout { size_t point_rows, point_slot, keys_a, keys_b, vals_a, vals_b, temp, total; };
static SbEmitLayout sb_emit_layout(int64_t N, int64_t R) {
    SbEmitLayout L;
    size_t o = 0;
    L.point_rows = o; o += sb_al(sizeof(int32_t) * (size_t)N);
    L.point_slot = o; o += sb_al(sizeof(int32_t) * (size_t)N);
    L.keys_a = o;     o += sb_al(sizeof(unsigned long long) * (size_t)R);
    L.keys_b = o;     o += sb_al(sizeof(unsigned long long) * (size_t)R);
    L.vals_a = o;     o += sb_al(sizeof(uint32_t) * (size_t)R);
    L.vals_b = o;     o += sb_al(sizeof(uint32_t) * (size_t)R);
    const size_t t1 = rsort_workspace(R), t2 = sizeof(int32_t) * scan_block_sums(N) + 256;
    L.temp = o;       o += sb_al(t1 > t2 ? t1 : t2);
    L.total = o + 256;
    return L;
}

static char* sb_base(void* workspace) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255); }

static bool sb_spec_ok(const Spec* sp) {
    return sp && sp->block_size > 0.0 && sp->stride > 0.0 && sp->padding >= 0.0 && (sp->count_form == 0 || sp->count_form == 1);
}

constexpr int64_t SB_MAX = ((int64_t)1 << 31) - 1;

}  // namespace crf

using namespace crf;

extern "C" size_t crfconv_sliding_blocks_workspace(int64_t N, int64_t S, int64_t cell_cap) {
    (void)N;
    if (S < 0 || cell_cap < 1 || cell_cap > SB_MAX) return 0;
    return sb_layout(S, cell_cap).total;
}

extern "C" int crfconv_sliding_blocks_count(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const crf_sliding_blocks_spec* spec,
                                            int64_t cell_cap, float* pos_min, float* limit, int64_t* totals, void* workspace,
                                            size_t workspace_bytes, crf_stream_t stream) {
    CRF_REQUIRE(pos && ptr && pos_min && limit && totals && workspace, CRF_ERR_ARG, "sliding_blocks_count: null pointer");
    CRF_REQUIRE(N >= 1 && N <= SB_MAX && S >= 1 && S <= SB_MAX, CRF_ERR_ARG, "sliding_blocks_count: N=%lld, S=%lld out of range", (long long)N,
                (long long)S);
    CRF_REQUIRE(cell_cap >= 1 && cell_cap <= SB_MAX, CRF_ERR_ARG, "sliding_blocks_count: cell_cap=%lld out of range", (long long)cell_cap);
    CRF_REQUIRE(sb_spec_ok(spec), CRF_ERR_ARG, "sliding_blocks_count: block_size and stride must be positive, padding non-negative, count_form 0 or 1");
    const SbLayout L = sb_layout(S, cell_cap);
    CRF_REQUIRE(workspace_bytes >= L.total, CRF_ERR_WORKSPACE, "sliding_blocks_count: workspace %zu < %zu", workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char* ws = sb_base(workspace);
    unsigned* bnd = reinterpret_cast<unsigned*>(ws + L.bnd);
    int32_t* dims = reinterpret_cast<int32_t*>(ws + L.dims);
    int64_t* cell_off = reinterpret_cast<int64_t*>(ws + L.cell_off);
    int32_t* count = reinterpret_cast<int32_t*>(ws + L.count);
    int32_t* core_count = reinterpret_cast<int32_t*>(ws + L.core_count);
    int32_t* keep = reinterpret_cast<int32_t*>(ws + L.keep);
    int32_t* kept_count = reinterpret_cast<int32_t*>(ws + L.kept_count);
    int32_t* rank = reinterpret_cast<int32_t*>(ws + L.rank);
    int32_t* row_off = reinterpret_cast<int32_t*>(ws + L.row_off);
    int32_t* sums = reinterpret_cast<int32_t*>(ws + L.sums);

    CRF_HIP(hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), st));
    CRF_HIP(hipMemsetAsync(bnd, 0xff, sizeof(unsigned) * 6 * (size_t)S, st));
    // count and core_count are neighbours in the layout: one fill.  keep / kept_count stay zero where sb_decide leaves early (a status).
    CRF_HIP(hipMemsetAsync(count, 0, L.rank - L.count, st));
    const dim3 blk(256), per_point((unsigned)cdiv(N, 256)), per_cell((unsigned)cdiv(cell_cap, 256));
    hipLaunchKernelGGL(sb_bounds_kernel<0>, dim3((unsigned)cdiv(N, SB_BOUNDS_PPB)), blk, 0, st, pos, N, ptr, (int)S, bnd, totals);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_grid_kernel, dim3(1), blk, 0, st, bnd, ptr, (int)S, *spec, cell_cap, pos_min, limit, dims, cell_off, totals);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_count_kernel, per_point, blk, 0, st, pos, N, ptr, (int)S, *spec, pos_min, dims, cell_off, totals, count, core_count);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_decide_kernel, per_cell, blk, 0, st, count, core_count, cell_cap, *spec, totals, keep, kept_count);
    CRF_LAUNCH_CHECK();
    exclusive_scan_i32(keep, rank, cell_cap, sums, st);
    CRF_LAUNCH_CHECK();
    exclusive_scan_i32(kept_count, row_off, cell_cap, sums, st);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" size_t crfconv_sliding_blocks_emit_workspace(int64_t N, int64_t n_rows) {
    if (N < 1 || N > SB_MAX || n_rows < 1 || n_rows > SB_MAX) return 0;
    return sb_emit_layout(N, n_rows).total;
}

extern "C" int crfconv_sliding_blocks_emit(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const crf_sliding_blocks_spec* spec,
                                           int64_t cell_cap, const float* pos_min, int64_t n_blocks, int64_t n_rows, void* workspace,
                                           size_t workspace_bytes, void* emit_workspace, size_t emit_workspace_bytes, int64_t* out_ptr,
                                           int64_t* rows, int64_t* indices, int8_t* mask, int64_t* batch, int64_t* scene, int32_t* cell,
                                           crf_stream_t stream) {
    CRF_REQUIRE(pos && ptr && pos_min && workspace && emit_workspace && out_ptr && rows && indices && mask && batch && scene && cell,
                CRF_ERR_ARG, "sliding_blocks_emit: null pointer");
    CRF_REQUIRE(N >= 1 && N <= SB_MAX && S >= 1 && S <= SB_MAX && cell_cap >= 1 && cell_cap <= SB_MAX, CRF_ERR_ARG,
                "sliding_blocks_emit: N=%lld, S=%lld, cell_cap=%lld out of range", (long long)N, (long long)S, (long long)cell_cap);
    CRF_REQUIRE(n_blocks >= 1 && n_blocks <= cell_cap && n_rows >= 1 && n_rows <= SB_MAX, CRF_ERR_ARG,
                "sliding_blocks_emit: n_blocks=%lld, n_rows=%lld out of range", (long long)n_blocks, (long long)n_rows);
    CRF_REQUIRE(sb_spec_ok(spec), CRF_ERR_ARG, "sliding_blocks_emit: bad spec");
    const SbLayout L = sb_layout(S, cell_cap);
    const SbEmitLayout E = sb_emit_layout(N, n_rows);
    CRF_REQUIRE(workspace_bytes >= L.total && emit_workspace_bytes >= E.total, CRF_ERR_WORKSPACE, "sliding_blocks_emit: workspace %zu < %zu or %zu < %zu",
                workspace_bytes, L.total, emit_workspace_bytes, E.total);
    hipStream_t st = as_stream(stream);
    char* ws = sb_base(workspace);
    char* ew = sb_base(emit_workspace);
    const int32_t* dims = reinterpret_cast<int32_t*>(ws + L.dims);
    const int64_t* cell_off = reinterpret_cast<int64_t*>(ws + L.cell_off);
    const int32_t* keep = reinterpret_cast<int32_t*>(ws + L.keep);
    const int32_t* rank = reinterpret_cast<int32_t*>(ws + L.rank);
    const int32_t* row_off = reinterpret_cast<int32_t*>(ws + L.row_off);
    int32_t* point_rows = reinterpret_cast<int32_t*>(ew + E.point_rows);
    int32_t* point_slot = reinterpret_cast<int32_t*>(ew + E.point_slot);
    auto* keys_a = reinterpret_cast<unsigned long long*>(ew + E.keys_a);
    auto* keys_b = reinterpret_cast<unsigned long long*>(ew + E.keys_b);
    uint32_t* vals_a = reinterpret_cast<uint32_t*>(ew + E.vals_a);
    uint32_t* vals_b = reinterpret_cast<uint32_t*>(ew + E.vals_b);
    void* temp = ew + E.temp;

    const dim3 blk(256), per_point((unsigned)cdiv(N, 256)), per_cell((unsigned)cdiv(cell_cap, 256)), per_row((unsigned)cdiv(n_rows, 256));
    hipLaunchKernelGGL(sb_recount_kernel, per_point, blk, 0, st, pos, N, ptr, (int)S, *spec, pos_min, dims, cell_off, keep, point_rows);
    CRF_LAUNCH_CHECK();
    exclusive_scan_i32(point_rows, point_slot, N, reinterpret_cast<int32_t*>(temp), st);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_emit_kernel, per_point, blk, 0, st, pos, N, ptr, (int)S, *spec, pos_min, dims, cell_off, keep, rank, point_slot,
                       n_rows, keys_a, vals_a);
    CRF_LAUNCH_CHECK();
    int bits = 0;                                          // of the largest block number
    while (bits < 64 && ((unsigned long long)(n_blocks - 1) >> bits) != 0ull) ++bits;
    const int where = rsort_pairs_u64(keys_a, vals_a, keys_b, vals_b, n_rows, 0, 8 * ((bits + 7) / 8), temp, st);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_blocks_kernel, per_cell, blk, 0, st, keep, rank, row_off, dims, cell_off, (int)S, n_blocks, n_rows, out_ptr, scene, cell);
    CRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sb_finish_kernel, per_row, blk, 0, st, where ? keys_b : keys_a, where ? vals_b : vals_a, n_rows, n_blocks, ptr, scene, rows,
                       indices, mask, batch);
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}

extern "C" int crfconv_sliding_blocks_features(const float* pos, int64_t N, const float* pos_min, const float* limit, int64_t S,
                                               const float* extra, int F, const int64_t* rows, const int64_t* batch, const int64_t* out_ptr,
                                               const int64_t* scene, int64_t n_blocks, int64_t n_rows, int form, float* block_bounds,
                                               float* pos_block, float* x, crf_stream_t stream) {
    CRF_REQUIRE(pos && pos_min && limit && rows && batch && out_ptr && scene && pos_block && x, CRF_ERR_ARG, "sliding_blocks_features: null pointer");
    CRF_REQUIRE(N >= 1 && N <= SB_MAX && S >= 1 && n_blocks >= 1 && n_blocks <= SB_MAX && n_rows >= 1 && n_rows <= SB_MAX, CRF_ERR_ARG,
                "sliding_blocks_features: sizes out of range");
    CRF_REQUIRE(F >= 0 && (F == 0 || extra), CRF_ERR_ARG, "sliding_blocks_features: F=%d needs extra", F);
    CRF_REQUIRE(form == 0 || (form == 1 && block_bounds), CRF_ERR_ARG, "sliding_blocks_features: form %d (block_bounds needed for form 1)", form);
    hipStream_t st = as_stream(stream);
    const dim3 blk(256), per_row((unsigned)cdiv(n_rows, 256));
    if (form == 0) {
        hipLaunchKernelGGL(sb_features_kernel<0>, per_row, blk, 0, st, pos, pos_min, limit, extra, F, rows, batch, scene, block_bounds, n_rows,
                           pos_block, x);
    } else {
        hipLaunchKernelGGL(sb_block_bounds_kernel, dim3((unsigned)n_blocks), blk, 0, st, pos, pos_min, rows, out_ptr, scene, block_bounds);
        CRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(sb_features_kernel<1>, per_row, blk, 0, st, pos, pos_min, limit, extra, F, rows, batch, scene, block_bounds, n_rows,
                           pos_block, x);
    }
    CRF_LAUNCH_CHECK();
    return CRF_OK;
}
