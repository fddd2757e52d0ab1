/* libcrfconv_amd.so -- part IoU of ragged batches of shapes (csrc/part_scores.hip), a PUBLIC part of the C ABI beside crfconv_amd.h,
 * crfconv_blocks.h, crfconv_block_votes.h and crfconv_grid.h: a C caller includes this file (it includes crfconv_amd.h for the status
 * codes and crf_stream_t).  Same machine-read dialect: crfconv_amd/_lib.py derives the ctypes signatures from THIS file into
 * _lib.PARTS_SIGNATURES / _lib.PARTS_RECORDS.  The entries stand here because the entry and record counts of crfconv_amd.h are pinned by
 * the host tests.
 *
 * Common arguments.  ptr [S + 1] int64: shape s owns rows ptr[s] .. ptr[s + 1] of the N rows; category [S] int64: its object category.
 * The part table in CSR form: parts_ptr [n_cat + 1] int32 and parts [parts_ptr[n_cat]] int32, the part labels of category c at
 * parts[parts_ptr[c] .. parts_ptr[c + 1]): distinct, ascending, inside [0, C), at least one per category.  1 <= C <= 64, 1 <= n_cat <= 64,
 * 0 <= N < 2^31, 1 <= S < 2^31.  Everything is device memory.  The table is the caller's to get right (crfconv_amd.utils.PartScores
 * checks it on the host); with a broken one the reads still stay inside parts [parts_ptr[n_cat]] and inside a score row.
 *
 * The prediction of row r of a shape of category c with part list L is y_pred[r], or from scores [N, C] float32:
 *   restrict_parts 1   the FIRST arg-max of scores[r, l] over l in L, in list order: the first part is the start value and a later one
 *                      replaces it only when strictly greater, so ties go to the lowest label and a NaN never wins
 *   restrict_parts 0   the first arg-max over all C columns by the same rule (what crfconv_confusion_accumulate does)
 * A row that no shape owns, and with restrict_parts 1 a row of a shape whose category is outside [0, n_cat), has the prediction -1. */
#ifndef CRFCONV_PARTS_H
#define CRFCONV_PARTS_H

#include "crfconv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the per-shape counters, [S, 3, C] int32.  0: a size out of range. */
size_t crfconv_part_scores_workspace(int64_t S, int C);

/* One update of the running part scores with a batch of S shapes.  y_true [N] int64; exactly one of y_pred [N] int64 and scores [N, C]
 * float32 is given, the other is NULL (restrict_parts is read with scores only); with N = 0 all three may be NULL.
 *
 * Per shape s of category c with list L, for each l in L the integers I_l = rows with t == l and p == l, T_l = rows with t == l,
 * P_l = rows with p == l, U_l = T_l + P_l - I_l; labels and predictions outside L or outside [0, C) match no part.  Then, in IEEE double,
 *   shape_iou[s] = (((0.0 + q_1) + q_2) + ..) / double(len(L)),   q_l = (double(I_l) + eps) / (double(U_l) + eps),   eps = 2^-23,
 * in list order with true divisions; an empty shape gives exactly 1.0.  In ascending s:  cat_sum[c] <- float32(double(cat_sum[c]) +
 * shape_iou[s]), one rounding per shape, and cat_num[c] += 1.  A shape whose category is outside [0, n_cat) or whose bounds are not
 * 0 <= ptr[s] <= ptr[s + 1] <= N gets shape_iou[s] = NaN, is not accumulated, and *bad grows by one; all reads stay inside the buffers
 * (with bounds that do not ascend the counts of the other shapes are memory-safe, not meaningful).
 *
 * Outputs: pred_out [N] int64 or NULL, the predictions; shape_iou [S] double; counts_out [S, 3, C] int32 or NULL: I, T, P per label,
 * zero for labels outside the shape's list; cat_sum [n_cat] float32, cat_num [n_cat] int32 and bad [1] int32 are read and written (the
 * running state).  workspace: crfconv_part_scores_workspace(S, C) bytes; not needed (NULL, 0) when counts_out is given, which then holds
 * the counters itself.
 *
 * A memset of the counters and two launches on `stream`: a count pass over fixed tiles of 128 rows of the flat batch (the grid depends on
 * N alone; integer atomics only, so the same bits in every run) and a finish pass of one workgroup in which every output word has one
 * writer.  No float atomics, no scratch memory, no host read, no allocation: capturable in a hipGraph. */
int crfconv_part_scores_update(const int64_t* y_true, const int64_t* y_pred, const float* scores, int64_t N, int C, const int64_t* ptr,
                               const int64_t* category, int64_t S, const int32_t* parts_ptr, const int32_t* parts, int n_cat,
                               int restrict_parts, void* workspace, size_t workspace_bytes, int64_t* pred_out, double* shape_iou,
                               int32_t* counts_out, float* cat_sum, int32_t* cat_num, int32_t* bad, crf_stream_t stream);

/* The prediction alone: pred_out [N] int64 from scores [N, C] float32, as above.  ONE launch (the count pass without its counters). */
int crfconv_part_predict(const float* scores, int64_t N, int C, const int64_t* ptr, const int64_t* category, int64_t S,
                         const int32_t* parts_ptr, const int32_t* parts, int n_cat, int restrict_parts, int64_t* pred_out,
                         crf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRFCONV_PARTS_H */
