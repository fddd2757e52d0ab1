/* libcrfconv_amd.so -- the sliding block split of scenes (csrc/blocks.hip), a PUBLIC part of the C ABI beside crfconv_amd.h: a C caller
 * includes this file (it includes crfconv_amd.h for the status codes and crf_stream_t).  Same machine-read dialect: crfconv_amd/_lib.py
 * derives the ctypes signatures and the record class from THIS file into _lib.BLOCKS_SIGNATURES / _lib.BLOCKS_RECORDS.  The entries stand
 * here and not in crfconv_amd.h because that header's entry and record counts are pinned by the existing host tests. */
#ifndef CRFCONV_BLOCKS_H
#define CRFCONV_BLOCKS_H

#include "crfconv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sliding XY blocks of the scenes of a RAGGED batch, csrc/blocks.hip (the process_raw_path bodies of datasets/scannet_dataset.py:58-117,
 * s3dis_dataset.py:119-171, semantic3d_dataset.py:107-157, npm3d_dataset.py:90-144).  pos [N, 3] float32, ptr [S + 1] device int64
 * (scene s = rows ptr[s] .. ptr[s + 1]), N < 2^31.  Per scene: a = pos - min(pos) (float32, one rounding), limit = max(a); block counts
 * per axis in double from the float32 limit, count_form 0: int(ceil((limit - block_size) / stride)) + 1, count_form 1:
 * int(ceil(limit - block_size) / stride) + 1, below 0 -> 0; block (i, j) starts at (i stride, j stride) in double and holds the points
 * with f32(beg - padding) <= a <= f32((beg + block_size) + padding) on x and y (float32 comparison), its core flag is the same test with
 * f32(beg) and f32(beg + block_size); a block is kept iff count >= min_points and double(core count) / double(count) >= proportion.
 * Kept blocks are numbered scene-major, then i, then j; rows inside a block ascend.
 *
 * crfconv_sliding_blocks_count enqueues the per-scene bounds (pos_min, limit [S, 3]), the grid (all scenes' cells in one flat numbering),
 * the per-cell counts (integer atomics) and the keep decision, and leaves totals [4] int64 on the device:
 *   totals[0] kept blocks   totals[1] their rows   totals[2] grid cells   totals[3] status, 0 = fine; bit 0: ptr does not start at 0,
 *   end at N or ascend; bit 1: more grid cells than cell_cap (call again with cell_cap >= totals[2]); bit 2: a scene with more than 2^22 blocks along an axis
 *   (up to there the candidate range each point tests is proven to hold all its blocks), or 2^31 grid cells or more in the batch.
 * With a status other than 0 nothing else was written.  The caller reads totals (its ONE host read), sizes the outputs and calls
 * crfconv_sliding_blocks_emit with the same arguments and workspace: every point writes its (block, row) pairs at a slot of its own,
 * a stable radix sort over the bits the block number needs groups them (rows of a block stay ascending), and out_ptr [n_blocks + 1],
 * rows / indices / batch [n_rows] int64, mask [n_rows] int8, scene [n_blocks] int64, cell [n_blocks, 2] int32 are written.  n_rows < 2^31.
 * Positions must be finite.  A scene's minimum that is a zero of both signs is taken as -0.0.
 * Deterministic: no float atomics, integer atomics only where the order cannot matter.  Workspace sizes: the two _workspace queries. */
typedef struct crf_sliding_blocks_spec {
    double block_size, stride, padding, proportion;
    int64_t min_points;
    int32_t count_form;
} crf_sliding_blocks_spec;
size_t crfconv_sliding_blocks_workspace(int64_t N, int64_t S, int64_t cell_cap);
int crfconv_sliding_blocks_count(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const crf_sliding_blocks_spec* spec,
                                 int64_t cell_cap, float* pos_min, float* limit, int64_t* totals, void* workspace,
                                 size_t workspace_bytes, crf_stream_t stream);
size_t crfconv_sliding_blocks_emit_workspace(int64_t N, int64_t n_rows);
int crfconv_sliding_blocks_emit(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const crf_sliding_blocks_spec* spec,
                                int64_t cell_cap, const float* pos_min, int64_t n_blocks, int64_t n_rows, void* workspace,
                                size_t workspace_bytes, void* emit_workspace, size_t emit_workspace_bytes, int64_t* out_ptr,
                                int64_t* rows, int64_t* indices, int8_t* mask, int64_t* batch, int64_t* scene, int32_t* cell,
                                crf_stream_t stream);

/* Features of the rows of a block split: pos_block [n_rows, 3] = a[rows] and x [n_rows, 3 + F]; extra [N, F] float32 or NULL (F = 0).
 *   form 0 (room)   x = cat(extra, a / limit), float32 division, IEEE where limit is 0
 *   form 1 (block)  x = cat(a - centre, extra), centre = (block_min + block_max) / 2 over the block's rows of a in float32, its z replaced
 *                   by block_min.z; block_bounds [n_blocks, 6] float32 is scratch for the minima and maxima (order-free reduction, one
 *                   workgroup per block)
 * batch [n_rows] and scene [n_blocks] as crfconv_sliding_blocks_emit wrote them. */
int crfconv_sliding_blocks_features(const float* pos, int64_t N, const float* pos_min, const float* limit, int64_t S, const float* extra,
                                    int F, const int64_t* rows, const int64_t* batch, const int64_t* out_ptr, const int64_t* scene,
                                    int64_t n_blocks, int64_t n_rows, int form, float* block_bounds, float* pos_block, float* x,
                                    crf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRFCONV_BLOCKS_H */
