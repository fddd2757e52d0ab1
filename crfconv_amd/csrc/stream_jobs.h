/* Entry points of libcrfconv_amd.so that only the Python package calls (crfconv_amd.ops.mlp): the job launches of the narrow row-streaming
 * MLP blocks.  They are NOT part of the public C ABI of include/crfconv_amd.h -- that header, its dialect and its counts stay as they are --
 * but they are declared in the same machine-read dialect: crfconv_amd/_lib.py derives their ctypes signatures and record classes from THIS
 * file into a second pair of tables (_lib.INTERNAL_SIGNATURES, _lib.INTERNAL_RECORDS).  Conventions (status codes, streams, workspaces) are
 * the public header's. */
#ifndef CRFCONV_STREAM_JOBS_H
#define CRFCONV_STREAM_JOBS_H

#include "../../include/crfconv_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- several INDEPENDENT narrow row-streaming MLP blocks per launch (round 31): unary_nn[i] and pairwise_nn[i] of a fine-level CRF
 * layer (models/continuous_crf_conv_big.py:56-60) are launches of a few hundred workgroups that wait on memory round trips, so two of
 * them side by side cost about the longer one.  jobs: host arrays of 1 .. 4 entries.  Each job runs exactly the workgroups, rows,
 * summation orders, records and workspace slabs of its own single call (the jobs' grids laid end to end): results are bit-identical.
 *   crfconv_linear_forward_jobs = crfconv_linear_forward(X, W, NULL, M, Ci, Co, 0, Y, stat_rec) per job, one launch
 *                                 (crfconv_linear_forward_jobs_supported: Ci, Co multiples of 4, Co <= 16, Ci <= 64)
 *   crfconv_mlp_backward_jobs   = crfconv_mlp_backward_add per job, two launches in all -- pass 1 of every job, then every dX product
 *                                 (dX may be NULL; dX_add may be NULL; dW NULL = deferred to crfconv_mlp_dw_jobs, else one more launch for
 *                                 that job).  tickets: 4 x crfconv_ticket_bytes() ZERO bytes owned by the stream, left zero -- one block
 *                                 of ticket words per job.  Shapes: both crfconv_mlp_backward_p1_jobs_supported and _dx_jobs_supported
 *                                 (Co in {4, 8, 16}). */
typedef struct { const float* X; const float* W; int64_t M; int Ci; int Co; float* Y; float* stat_rec;
                 /* tiled != 0: this job is crfconv_gemm_stats(X, W, M, Co, Ci, Y, stat_rec) instead -- a block BELOW the row-streaming forms'
                  * switch-over riding the launch of its partner above it (the level-1 CRF layer's pair).  Up to 2 such jobs, first in the
                  * array, with at least one row-streaming job behind them; same tiles, summation order and records as crfconv_gemm_stats
                  * (crfconv_linear_forward_jobs_tiled_supported: the 32 x 32 tile class, widths multiples of 4). */
                 int tiled;
} crf_linear_job;
int crfconv_linear_forward_jobs_supported(int64_t M, int Ci, int Co);
int crfconv_linear_forward_jobs_tiled_supported(int64_t M, int Ci, int Co);
int crfconv_linear_forward_jobs(const crf_linear_job* jobs, int njobs, crf_stream_t stream);
typedef struct { const float* gA; const float* Y; const float* X; const float* W; const float* coef; float slope; int64_t M; int Ci; int Co;
                 const float* dX_add; float* dX; float* dW; float* dgamma; float* dbeta; void* workspace; size_t workspace_bytes;
} crf_mlp_stream_bwd_job;
int crfconv_mlp_backward_p1_jobs_supported(int64_t M, int Ci, int Co);
int crfconv_mlp_backward_dx_jobs_supported(int64_t M, int Ci, int Co);
int crfconv_mlp_backward_jobs(const crf_mlp_stream_bwd_job* jobs, int njobs, unsigned* tickets, crf_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* CRFCONV_STREAM_JOBS_H */
