// Device functions of the unprocess chain (isp/unprocess_np.py:53-80, 177-181), shared by adaisp_unprocess
// (isp_unprocess.hip: all three channels of a pixel) and adaisp_unprocess_bayer (isp_sensor.hip: the one channel the
// colour filter keeps). Both build a pixel from the same functions below, in the same order, so a kept channel is the
// fp32 value the three-channel kernel writes for it by construction: the tone table, the colour matrix rows and the
// saturation mask (which needs all three rows), then per channel the gain, the clips and the noise.
//
// The normals come from Philox4x32-10 (Salmon et al., SC'11) keyed by (seed, image serial) with the pixel's index inside
// the un-padded image as the counter, then Box-Muller: an image's noise depends on (seed, serial) alone, not on its
// batch, its place in it, its staging offset or the launch geometry.
#pragma once
#include "isp_internal.h"

namespace adaisp {
namespace {

struct Philox4 { uint32_t x, y, z, w; };

__device__ __forceinline__ Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = Philox4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// 24-bit uniforms are exact in fp32: u1 in (0, 1] (log never sees 0), u2 in [0, 1)
__device__ __forceinline__ float unit_open0(uint32_t v) { return (float)((v >> 8) + 1u) * 0x1.0p-24f; }
__device__ __forceinline__ float unit_closed0(uint32_t v) { return (float)(v >> 8) * 0x1.0p-24f; }

// the four words behind the three N(0, 1) draws of pixel `idx` of image (seed, serial)
__device__ __forceinline__ Philox4 noise_words(uint64_t seed, uint64_t serial, uint32_t idx) {
    return philox4x32_10(Philox4{idx, (uint32_t)(serial >> 32), (uint32_t)(seed >> 32), 0u}, (uint32_t)seed,
                         (uint32_t)serial);
}

// Box-Muller on one pair of words: radius * (cos, sin)(2 pi u2)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float* c, float* s) {
    float sn, cs;
    const float r = sqrtf(-2.0f * logf(unit_open0(a)));
    sincospif(2.0f * unit_closed0(b), &sn, &cs);
    *c = r * cs;
    *s = r * sn;
}

// three N(0, 1) draws for pixel `idx` of image (seed, serial): Box-Muller on (x, y) gives two, on (z, w) one
__device__ __forceinline__ void normals3(uint64_t seed, uint64_t serial, uint32_t idx, float n[3]) {
    const Philox4 r = noise_words(seed, serial, idx);
    float unused;
    box_muller(r.x, r.y, &n[0], &n[1]);
    box_muller(r.z, r.w, &n[2], &unused);
}

// the c-th of normals3's draws alone: the same words, the one Box-Muller pair that holds it
__device__ __forceinline__ float normal_of(uint64_t seed, uint64_t serial, uint32_t idx, int c) {
    const Philox4 r = noise_words(seed, serial, idx);
    float cs, sn;
    box_muller(c == 2 ? r.z : r.x, c == 2 ? r.w : r.y, &cs, &sn);
    return c == 1 ? sn : cs;
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// inverse_smoothstep then gamma_expansion (:53-61) of one 8-bit value at the image's pre-scale
__device__ __forceinline__ float tone_gamma(int u8, float prescale) {
    const float x = clip01((float)u8 / 255.0f * prescale);
    return powf(fmaxf(0.5f - sinf(asinf(1.0f - 2.0f * x) / 3.0f), 1e-8f), 2.2f);
}

// apply_ccm (:63-68) of t = tone_gamma of R, G, B, and safe_invert_gains' mask (:70-80) from its three rows
__device__ __forceinline__ float ccm_and_mask(const float t[3], const float* __restrict__ p, float y[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        y[c] = (t[0] * p[ADAISP_UNP_CCM + 3 * c] + t[1] * p[ADAISP_UNP_CCM + 3 * c + 1]) + t[2] * p[ADAISP_UNP_CCM + 3 * c + 2];
    const float gray = ((y[0] + y[1]) + y[2]) / 3.0f;
    const float m = fmaxf(gray - 0.9f, 0.0f) / 0.1f;
    return m * m;
}

// one channel after the matrix: masked gain `g`, clip, brightness ratio
__device__ __forceinline__ float gain_clip(float yc, float mask, float g, const float* __restrict__ p) {
    return clip01(yc * fmaxf(mask + (1.0f - mask) * g, g)) * p[ADAISP_UNP_RATIO];
}

// add_read_and_shot_noise (:177-181) with the N(0, 1) draw `n`, and the clip after it
__device__ __forceinline__ float shot_read(float x, float n, const float* __restrict__ p) {
    return clip01(x + n * sqrtf(x * p[ADAISP_UNP_SHOT] + p[ADAISP_UNP_READ]));
}

// the rest of the chain for one pixel: t = tone_gamma of R, G, B in, the output RGB out
template <bool NOISE>
__device__ __forceinline__ void unprocess_px(const float t[3], float v[3], const float* __restrict__ p, uint64_t seed,
                                             uint64_t serial, uint32_t idx) {
    float y[3];
    const float mask = ccm_and_mask(t, p, y);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (NOISE) normals3(seed, serial, idx, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = gain_clip(y[c], mask, p[ADAISP_UNP_GAIN + c], p);
        if (NOISE) x = shot_read(x, n[c], p);
        v[c] = x;
    }
}

// channel c of unprocess_px alone: every row of the matrix (the mask needs them), one gain, one clip, one normal
template <bool NOISE>
__device__ __forceinline__ float unprocess_ch(const float t[3], int c, const float* __restrict__ p, uint64_t seed,
                                              uint64_t serial, uint32_t idx) {
    float y[3];
    const float mask = ccm_and_mask(t, p, y);
    float x = gain_clip(c == 0 ? y[0] : (c == 1 ? y[1] : y[2]), mask, p[ADAISP_UNP_GAIN + c], p);
    if (NOISE) x = shot_read(x, normal_of(seed, serial, idx, c), p);
    return x;
}

}  // namespace
}  // namespace adaisp
