// What the two augmentation units share: augment.hip (dense crops [B, N, 3]) and augment_segments.hip (a ragged batch pos [N, 3] +
// ptr [S + 1]).  The host check of the spec fields both records carry (aug_check_spec), the per-cloud draws, the per-point steps
// (rotate and scale; flip, then clamped noise) and the params_out row.  Both units call the SAME device functions, so cloud b of a
// ragged batch applies what Compose.draws(seed, counter, S) predicts for row b of a dense one, one singly rounded operation at a time.
// `Spec` is crf_augment_spec or crf_augment_segments_spec (include/crfconv_amd.h): the fields read here carry the same names in both.
#pragma once
#include <cmath>

#include "common.hpp"

namespace crf {

constexpr unsigned long long AUG_DOMAIN = 0xA0761D6478BD642Full;       // separates these draws from the subsets' / dropout's
constexpr int AUG_SLOT_NOISE = 8;                                      // slots 0 .. 7 per cloud, 8 + 3 point + axis per point

__device__ __forceinline__ unsigned long long aug_hash(unsigned long long seed, unsigned long long ctr, unsigned long long cloud,
                                                       unsigned long long slot) {
    unsigned long long z = (seed ^ AUG_DOMAIN) + 0x9E3779B97F4A7C15ull * (ctr + 1ull) + cloud * 0xC2B2AE3D27D4EB4Full
                           + slot * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float aug_u24(unsigned long long h) { return (float)(unsigned)(h >> 40) * 5.9604644775390625e-8f; }   // [0, 1)

// The fields of crf_augment_spec, which crf_augment_segments_spec carries too: CRF_OK, or CRF_ERR_ARG with the message set.
template <class Spec>
inline int aug_check_spec(const Spec& sp) {
    CRF_REQUIRE(sp.rotate_axis >= -1 && sp.rotate_axis <= 2, CRF_ERR_ARG, "rotate_axis=%d outside {-1, 0, 1, 2}", sp.rotate_axis);
    CRF_REQUIRE(std::isfinite(sp.deg_lo) && std::isfinite(sp.deg_hi) && sp.deg_lo <= sp.deg_hi, CRF_ERR_ARG,
                "rotation range [%g, %g]", (double)sp.deg_lo, (double)sp.deg_hi);
    CRF_REQUIRE(std::isfinite(sp.scale_lo) && std::isfinite(sp.scale_span) && sp.scale_span >= 0.f, CRF_ERR_ARG,
                "scale range lo=%g span=%g", (double)sp.scale_lo, (double)sp.scale_span);
    CRF_REQUIRE(sp.flip_axes >= 0 && sp.flip_axes <= 7, CRF_ERR_ARG, "flip_axes=%d outside [0, 7]", sp.flip_axes);
    CRF_REQUIRE((sp.scale == 0 || sp.scale == 1) && (sp.noise == 0 || sp.noise == 1) && (sp.drop == 0 || sp.drop == 1), CRF_ERR_ARG,
                "scale / noise / drop flags must be 0 or 1");
    CRF_REQUIRE(sp.sigma >= 0.f && sp.clip >= 0.f && std::isfinite(sp.sigma) && std::isfinite(sp.clip), CRF_ERR_ARG,
                "noise sigma=%g clip=%g", (double)sp.sigma, (double)sp.clip);
    CRF_REQUIRE(sp.drop_p >= 0.f && sp.drop_p <= 1.f, CRF_ERR_ARG, "drop probability %g outside [0, 1]", (double)sp.drop_p);
    return CRF_OK;
}

struct AugParams {
    float c, s, sc0, sc1, sc2;
    int flip, keep;
};

// What cloud b applies: the draws, or params_in [B, 8] when given; a disabled step is the identity.
template <class Spec>
__device__ __forceinline__ AugParams aug_cloud_params(const Spec& sp, unsigned long long seed, unsigned long long ctr, int b,
                                                     const float* __restrict__ params_in) {
    AugParams P{1.f, 0.f, 1.f, 1.f, 1.f, 0, 1};
    if (params_in != nullptr) {
        const float* q = params_in + (size_t)b * 8;
        if (sp.rotate_axis >= 0) { P.c = q[0]; P.s = q[1]; }
        if (sp.scale) { P.sc0 = q[2]; P.sc1 = q[3]; P.sc2 = q[4]; }
        P.flip = (int)q[5] & sp.flip_axes;
        if (sp.drop) P.keep = q[6] != 0.f ? 1 : 0;
        return P;
    }
    if (sp.rotate_axis >= 0) {            // double: the host twin's float64 cos / sin give the same float32 (to an ulp)
        const double u = (double)aug_u24(aug_hash(seed, ctr, b, 0));
        const double deg = (double)sp.deg_lo + ((double)sp.deg_hi - (double)sp.deg_lo) * u;
        const double rad = deg * 0.017453292519943295;
        P.c = (float)cos(rad);
        P.s = (float)sin(rad);
    }
    if (sp.scale) {
        P.sc0 = add_rn(sp.scale_lo, mul_rn(aug_u24(aug_hash(seed, ctr, b, 1)), sp.scale_span));
        P.sc1 = add_rn(sp.scale_lo, mul_rn(aug_u24(aug_hash(seed, ctr, b, 2)), sp.scale_span));
        P.sc2 = add_rn(sp.scale_lo, mul_rn(aug_u24(aug_hash(seed, ctr, b, 3)), sp.scale_span));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (((sp.flip_axes >> i) & 1) && aug_u24(aug_hash(seed, ctr, b, 4 + i)) < 0.5f) P.flip |= 1 << i;
    if (sp.drop) P.keep = aug_u24(aug_hash(seed, ctr, b, 7)) < sp.drop_p ? 0 : 1;
    return P;
}

// pos @ M (PyG's matrix about `axis`: x_a' = c x_a - s x_b, x_b' = s x_a + c x_b with (a, b) = (axis + 1, axis + 2) mod 3), then the
// scales when `scale` is set.  ONE instruction sequence for every pass that needs it (singly rounded: a max pass and the apply pass
// agree bit for bit).
__device__ __forceinline__ void aug_rotate_scale(int ax, int scale, const AugParams& P, float& x, float& y, float& z) {
    if (ax >= 0) {
        const float xa = ax == 2 ? x : (ax == 0 ? y : z), xb = ax == 2 ? y : (ax == 0 ? z : x);
        const float ra = sub_rn(mul_rn(P.c, xa), mul_rn(P.s, xb)), rb = add_rn(mul_rn(P.s, xa), mul_rn(P.c, xb));
        const float nx = ax == 2 ? ra : (ax == 1 ? rb : x);
        const float ny = ax == 2 ? rb : (ax == 0 ? ra : y);
        const float nz = ax == 0 ? rb : (ax == 1 ? ra : z);
        x = nx; y = ny; z = nz;
    }
    if (scale) {
        x = mul_rn(x, P.sc0);
        y = mul_rn(y, P.sc1);
        z = mul_rn(z, P.sc2);
    }
}
template <class Spec>
__device__ __forceinline__ void aug_rotate_scale(const Spec& sp, const AugParams& P, float& x, float& y, float& z) {
    aug_rotate_scale(sp.rotate_axis, sp.scale, P, x, y, z);
}

// sigma N(0, 1) of (cloud, slot), slot = AUG_SLOT_NOISE + 3 point + axis; Box-Muller: u1 in (0, 1], u2 in [0, 1).  Before the clamp.
__device__ __forceinline__ float aug_noise_draw(float sigma, unsigned long long seed, unsigned long long ctr, int b,
                                                unsigned long long slot) {
    const unsigned long long h = aug_hash(seed, ctr, b, slot);
    const float u1 = (float)((unsigned)(h >> 40) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)((unsigned)(h >> 8) & 0xFFFFFFu) * 5.9604644775390625e-8f;
    return sigma * (sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2));
}

// pos + clamp(noise, -clip, clip)
__device__ __forceinline__ float aug_add_noise(float p, float nz, float clip) { return add_rn(p, fminf(fmaxf(nz, -clip), clip)); }

// One rotated and scaled point: a flipped axis i becomes cm_i - p_i (cm_i = the cloud's max of that coordinate), then the clamped
// noise nz[0 .. 3) per axis (read only when sp.noise is set).
template <class Spec>
__device__ __forceinline__ void aug_flip_noise(const Spec& sp, const AugParams& P, float cm0, float cm1, float cm2, const float* nz,
                                               float& x, float& y, float& z) {
    if (P.flip & 1) x = sub_rn(cm0, x);
    if (P.flip & 2) y = sub_rn(cm1, y);
    if (P.flip & 4) z = sub_rn(cm2, z);
    if (sp.noise) {
        x = aug_add_noise(x, nz[0], sp.clip);
        y = aug_add_noise(y, nz[1], sp.clip);
        z = aug_add_noise(z, nz[2], sp.clip);
    }
}

// params_out row o [8] <- (cos, sin, sx, sy, sz, flip mask, keep, c_max) as applied; c_max: the cloud's maximum cm_i of the lowest
// flipped axis, 0 without a flip or for a cloud without points (`empty`).  The selection stands here, after the stores, and not at the
// call: handed the finished c_max, aug_segments_kernel allocates 97 VGPRs (4 waves per SIMD) instead of 96 (5).
__device__ __forceinline__ void aug_write_params(float* o, const AugParams& P, float cm0, float cm1, float cm2, bool empty) {
    o[0] = P.c; o[1] = P.s; o[2] = P.sc0; o[3] = P.sc1; o[4] = P.sc2; o[5] = (float)P.flip; o[6] = (float)P.keep;
    o[7] = empty ? 0.f : ((P.flip & 1) ? cm0 : ((P.flip & 2) ? cm1 : ((P.flip & 4) ? cm2 : 0.f)));
}

}  // namespace crf
