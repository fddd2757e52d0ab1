/* C ABI of libcrfconv_amd.so, the entries of csrc/augment_segments.hip: the transforms ahead of the sparse networks on a ragged batch.
 * Included by crfconv_amd.h (include that one); written in the same dialect, and read by crfconv_amd/_lib.py with the same parser. */
#ifndef CRFCONV_AMD_SEGMENTS_H
#define CRFCONV_AMD_SEGMENTS_H

/* The transforms ahead of the sparse networks on a RAGGED batch, csrc/augment_segments.hip, in place: pos [N, 3] float32, norm
 * [N, 3] or NULL, x [N, C] or NULL (C = 3: [pos]; C = 6: [pos, rgb], or [pos, norm] when x_norm = 1, which needs norm), and the S
 * clouds of a device ptr [S + 1] (cloud b = rows ptr[b] .. ptr[b + 1], kept inside [0, N]).  Per cloud, every step optional:
 *   center     (center = 1) pos -= c, c = the cloud's mean, summed in double in a fixed order of the LOCAL rows, rounded once
 *   normalize  (normalize = 1) pos *= k, k = (1 / max |pos|) * 0.999999f over the centred cloud; k = 0 where that maximum is 0
 *              (one point, coincident points: the zeros stay; PyG's NormalizeScale writes NaN there)
 *   rotate, scale, flip, noise, drop   as crfconv_augment: the same draws of (seed, *counter, cloud = position in ptr) and the
 *              same singly rounded operations; the noise hash takes the LOCAL row
 *   normals    rotate n <- n @ M; scale n_i <- n_i / s_i, renormalised to unit length (a zero normal stays zero); flip of axis i
 *              n_i <- -n_i; center, normalize and noise leave them alone
 *   x[:, 0:3] <- pos; x[:, 3:6] <- norm (x_norm = 1), or <- 0 on a dropped rgb.
 * params_in [S, 8] / noise_in [N, 3] / params_out [S, 8] as in crfconv_augment; stats_out [S, 4] (or NULL) <- (cx, cy, cz, k) as
 * applied (0, 0, 0 without center, k = 1 without normalize).  ONE launch, one workgroup per cloud, no workspace, no atomics:
 * bitwise deterministic, a cloud's output does not depend on the rest of the batch, capturable.  A cloud of 0 rows writes only its
 * params_out / stats_out rows. */
typedef struct crf_augment_segments_spec {
    int32_t center, normalize;
    int32_t rotate_axis;
    float deg_lo, deg_hi;
    int32_t scale;
    float scale_lo, scale_span;
    int32_t flip_axes;
    int32_t noise;
    float sigma, clip;
    int32_t drop;
    float drop_p;
    int32_t x_norm;
} crf_augment_segments_spec;
int crfconv_augment_segments(float* pos, float* norm, float* x, int64_t N, int C, const int64_t* ptr, int64_t S,
                             const crf_augment_segments_spec* spec, uint64_t seed, const int64_t* counter, const float* params_in,
                             const float* noise_in, float* params_out, float* stats_out, crf_stream_t stream);

/* PyG FixedPoints(num, replace, allow_duplicates) per cloud of a ragged batch, csrc/augment_segments.hip: cloud b (rows ptr[b] ..
 * ptr[b + 1] of N) receives m_b = out_ptr[b + 1] - out_ptr[b] picks, GLOBAL rows, at index[out_ptr[b] ..] (index [M] int64; ptr,
 * out_ptr [S + 1] device int64).  h(b, j): splitmix64's finisher over (seed ^ a domain constant, *counter, b, j); *counter is a
 * device word.
 *   mode 0 (replace)             pick t = ((h(b, t) >> 32) * n_b) >> 32
 *   mode 1 (without replacement) the rows with the min(m_b, n_b) smallest keys h(b, j), ties to the lower j, in ascending row
 *                                order; slots beyond n_b hold -1
 *   mode 2 (allow_duplicates)    floor(m_b / n_b) whole copies of the cloud in row order, then mode 1 for the remainder
 * An empty cloud with m_b > 0 writes -1.  One launch, one workgroup per cloud.  Host twin: transforms.FixedPoints.draws. */
int crfconv_fixed_points(const int64_t* ptr, const int64_t* out_ptr, int64_t S, int64_t N, int64_t M, int mode, uint64_t seed,
                         const int64_t* counter, int64_t* index, crf_stream_t stream);

#endif /* CRFCONV_AMD_SEGMENTS_H */
