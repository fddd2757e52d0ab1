/* libcrfconv_amd.so -- voxel-grid subsampling of a ragged batch of clouds on the device (csrc/grid_subsample.hip), a PUBLIC part of the C
 * ABI beside crfconv_amd.h: a C caller includes this file (it includes crfconv_amd.h for the status codes and crf_stream_t).  Same
 * machine-read dialect: crfconv_amd/_lib.py derives the ctypes signatures from THIS file into _lib.GRID_SIGNATURES / _lib.GRID_RECORDS.
 * The entries stand here and not in crfconv_amd.h because that header's entry and record counts are pinned by the host tests. */
#ifndef CRFCONV_GRID_H
#define CRFCONV_GRID_H

#include "crfconv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Grid subsampling (utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:5-106) of every cloud of a RAGGED batch in
 * one call: pos [N, 3] float32, ptr [S + 1] device int64 (cloud s = rows ptr[s] .. ptr[s + 1], an empty cloud repeats an entry),
 * feats [N, F] float32 or NULL (F = 0), labels [N, L] int32 or NULL (L = 0), size > 0 the voxel edge; 1 <= N < 2^31, S >= 1.  All
 * pointers are device pointers.  Each cloud has the origin and grid dimensions of its own bounding box, in the reference's float32
 * operations; a voxel's output row is the barycentre of its points (float32 sum in ascending row order, times float32(1.0 / n)), the mean
 * of their features (the same sum, divided by float32(n)) and per label column the most frequent label, the smallest one on a tie.
 * Rows come cloud by cloud and in ascending voxel key iX + NX iY + NX NY iZ inside a cloud: for one cloud the bits are those of
 * crfconv_grid_subsample.
 *
 * Written: out_pos [cap, 3], out_feats [cap, F], out_labels [cap, L] (rows 0 .. M), out_ptr [S + 1] int64 (cloud s = output rows
 * out_ptr[s] .. out_ptr[s + 1]), inverse [N] int64 (the output row of every input row's voxel), counts [cap] int32 (points per voxel),
 * and totals [2] int64 in device memory: totals[0] = M, the number of voxels, totals[1] = status, 0 = fine; bit 0: ptr does not start at
 * 0, end at N or ascend; bit 2: S > 1 and the clouds' cell counts NX NY NZ do not fit one 64-bit key together (one cloud alone keeps the
 * reference's wrap-around).  With a status other than 0, M is 0 and nothing else was written.  Rows at and past cap are not written: with
 * cap >= N that cannot happen; otherwise the caller compares totals[0] with cap.  out_ptr, inverse and counts may be NULL (not written).
 *
 * The entry enqueues its launches on `stream` and returns: no allocation, no synchronisation, no host read; the caller reads totals.
 * Deterministic: a stable radix sort puts every voxel's points in ascending row order, every output word has one writer, and the only
 * atomics are the integer minima of the bounds pass.  Positions must be finite.  Workspace: the _workspace query (0: sizes out of range). */
size_t crfconv_grid_subsample_segments_workspace(int64_t N, int64_t S);
int crfconv_grid_subsample_segments(const float* pos, int64_t N, const int64_t* ptr, int64_t S, const float* feats, int F,
                                    const int32_t* labels, int L, float size, int64_t cap, void* workspace, size_t workspace_bytes,
                                    float* out_pos, float* out_feats, int32_t* out_labels, int64_t* out_ptr, int64_t* inverse,
                                    int32_t* counts, int64_t* totals, crf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRFCONV_GRID_H */
