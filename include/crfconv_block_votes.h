/* libcrfconv_amd.so -- per-block scores merged back onto the points of the scenes (csrc/block_votes.hip), a PUBLIC part of the C ABI beside
 * crfconv_amd.h and crfconv_blocks.h: a C caller includes this file (it includes crfconv_amd.h for the status codes and crf_stream_t).
 * Same machine-read dialect: crfconv_amd/_lib.py derives the ctypes signatures from THIS file into _lib.VOTES_SIGNATURES /
 * _lib.VOTES_RECORDS.  The entries stand here because the entry and record counts of the other two headers are pinned by the host tests. */
#ifndef CRFCONV_BLOCK_VOTES_H
#define CRFCONV_BLOCK_VOTES_H

#include "crfconv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The inverse table of a block split (crfconv_sliding_blocks_emit): rows [R] int64, the point (0 <= rows[r] < N) of every block row, and
 * mask [R] int8, the core flag of the row.  rev_ptr [N + 1] int64 and rev_rows [R] int32 receive, for every point p, the block rows r
 * with rows[r] == p, ASCENDING in r, at rev_rows[rev_ptr[p] .. rev_ptr[p + 1]); bit 31 of an entry is the row's core flag (mask != 0),
 * bits 0..30 the row.  1 <= R < 2^31, 1 <= N < 2^31.  A stable radix sort of (key = rows[r], value = r) over the bytes N - 1 needs, then
 * every sorted item writes the rev_ptr entries between its predecessor's key and its own: no atomics, the same bits in every run.  A
 * value of rows outside [0, N) is taken as the nearest point (memory-safe, not meaningful).  Workspace: the _workspace query (0: sizes
 * out of range). */
size_t crfconv_block_reverse_workspace(int64_t N, int64_t R);
int crfconv_block_reverse(const int64_t* rows, int64_t R, int64_t N, const int8_t* mask, void* workspace, size_t workspace_bytes,
                          int64_t* rev_ptr, int32_t* rev_rows, crf_stream_t stream);

/* One update of the per-point sums: scores [R_part, C] float32 are the scores of block rows row_offset .. row_offset + R_part
 * (0 <= row_offset, row_offset + R_part <= R), 1 <= C <= 64.  For every point p the rows of its list that lie in that range and pass
 * `core` are taken in ascending order:
 *   core 0 (all)     every row
 *   core 1 (only)    rows with the core flag
 *   core 2 (prefer)  rows with the core flag if p has one ANYWHERE in its list (not only in the range), every row otherwise
 * s = ((t_1 + t_2) + t_3) + .. in float32, one singly rounded add per row, t = scores[r - row_offset, c], or expf of it (use_exp = 1);
 * then sums[p, c] <- sums[p, c] + s (one float32 add) and count[p] += the number of rows used.  A point without such a row is not
 * written.  sums [N, C] float32, count [N] int32.  ONE launch, one thread per (point, class): no atomics, every output word has one
 * writer, no scratch memory, no host read -- capturable in a hipGraph.  rev_ptr / rev_rows as crfconv_block_reverse wrote them (entries
 * are kept inside [0, R) when read). */
int crfconv_block_votes_update(const float* scores, int64_t R_part, int64_t row_offset, int C, const int64_t* rev_ptr,
                               const int32_t* rev_rows, int64_t R, int64_t N, int core, int use_exp, float* sums, int32_t* count,
                               crf_stream_t stream);

/* scores_out [N, C] float32 <- sums (reduce 0) or sums / float32(count), one correctly rounded division (reduce 1); pred [N] int64 <- the
 * FIRST arg-max of sums[p, 0..C) (ties go to the lowest class, as crfconv_vote_confusion).  Where count[p] == 0 the row is zero and
 * pred[p] = fill.  ONE launch: one thread per (point, class) writes the scores, the thread of class 0 walks the C sums for the arg-max. */
int crfconv_block_votes_result(const float* sums, const int32_t* count, int64_t N, int C, int reduce, int64_t fill, float* scores_out,
                               int64_t* pred, crf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRFCONV_BLOCK_VOTES_H */
