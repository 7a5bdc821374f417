// Filter arithmetic shared by the forward kernels and the two gradient families of libadaisp.so. The gradients recompute
// each pixel's forward value to gate on the output clip, so that value must match the forward kernel's to the last bit:
// every expression that more than one translation unit evaluates lives here once. The library is built with
// -ffp-contract=off, so operand order and parentheses below are the rounding sequence.
#pragma once
#include "isp_internal.h"

namespace adaisp {

// torch.remainder for floats: result takes the sign of the divisor.
__device__ __forceinline__ float py_mod(float a, float m) {
    float r = fmodf(a, m);
    if (r != 0.0f && (r < 0.0f)) r += m;   // m > 0 here
    return r;
}

// torch 'reflect' padding index (edge not repeated); valid for -n < i < 2n-1.
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// torch.roll's circular index
__device__ __forceinline__ int wrap(int v, int n) {
    v %= n;
    return v < 0 ? v + n : v;
}

// pass-through masks of a clamp to [0, 1] (torch.clip backward: the closed interval); gate01 only with ADAISP_CLIP01 set
__device__ __forceinline__ float in01(float v) { return (v >= 0.0f && v <= 1.0f) ? 1.0f : 0.0f; }
__device__ __forceinline__ float gate01(float f, bool clip) { return (!clip || (f >= 0.0f && f <= 1.0f)) ? 1.0f : 0.0f; }

__device__ __forceinline__ float lum_27_67_06(float r, float g, float b) {  // isp/filters.py:12-14
    return (0.27f * r + 0.67f * g) + 0.06f * b;
}

// rgb_to_luminance of the denoiser (denoise.py:11-17), applied to the clamped colour
constexpr float kNlmLuma[3] = {0.299f, 0.587f, 0.114f};
__device__ __forceinline__ float nlm_luma(float r, float g, float b) {
    return (kNlmLuma[0] * r + kNlmLuma[1] * g) + kNlmLuma[2] * b;
}

// Full-colour term of SaturationPlus (isp/filters.py:546-560 with rgb2hsv :445-478 and hsv2rgb :481-533) of a pixel that is
// already clamped to [0, 1]: the saturation boosted, the colour back from HSV.
__device__ __forceinline__ void satplus_full(float r, float g, float b, float& fr, float& fg, float& fb) {
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    const float d = (mx - mn) + 1e-8f;
    // sequential masked overwrite: B branch, then G, then R (so ties resolve R > G > B), then grey
    float hue = 0.0f;
    if (b == mx) hue = 4.0f + (r - g) / d;
    if (g == mx) hue = 2.0f + (b - r) / d;
    if (r == mx) hue = py_mod((g - b) / d, 6.0f);
    if (mn == mx) hue = 0.0f;
    hue = hue / 6.0f;
    float s = (mx - mn) / (mx + 1e-8f);
    if (mx == 0.0f) s = 0.0f;
    const float es = s + (1.0f - s) * (0.5f - fabsf(0.5f - mx)) * 0.8f;
    // hsv2rgb
    const float h = py_mod(hue, 1.0f), s2 = clamp01(es), v2 = clamp01(mx);
    const float h6 = h * 6.0f, hi = floorf(h6), f = h6 - hi;
    const float pp = v2 * (1.0f - s2), qq = v2 * (1.0f - (f * s2)), tt = v2 * (1.0f - ((1.0f - f) * s2));
    fr = fg = fb = 0.0f;
    if (hi == 0.0f) { fr = v2; fg = tt; fb = pp; }
    else if (hi == 1.0f) { fr = qq; fg = v2; fb = pp; }
    else if (hi == 2.0f) { fr = pp; fg = v2; fb = tt; }
    else if (hi == 3.0f) { fr = pp; fg = qq; fb = v2; }
    else if (hi == 4.0f) { fr = tt; fg = pp; fb = v2; }
    else if (hi == 5.0f) { fr = v2; fg = pp; fb = qq; }
}

// CCM (isp/filters.py:703-708): the rows of the 3x3 parameters divided by their sums `rs`
__device__ __forceinline__ void ccm_rows(const float* p, float (&m)[3][3], float (&rs)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rs[i] = (p[3 * i] + p[3 * i + 1]) + p[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[i][j] = p[3 * i + j] / rs[i];
    }
}

// _get_gaussian_kernel1d (isp/sharpen.py:15-23): g1[i] = exp(-0.5 * ((i - 2) / sigma)^2), i = 0..4; returns their sum
__device__ __forceinline__ float usm_gauss(float sigma, float (&g1)[5]) {
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float t = (float)(i - 2) / sigma;
        g1[i] = expf(-0.5f * (t * t));
        sum += g1[i];
    }
    return sum;
}

// Per-image stencil weights; returns the filter's amount. R = 2: the unsharp mask's normalised 5x5 gaussian (sigma p[0],
// amount p[1]); R = 1: the 3x3 sharpen pair's ones(3,3) with centre 5, divided by its sum (amount p[0]).
template <int R>
__device__ __forceinline__ float stencil_weights(const float* p, float (&w)[2 * R + 1][2 * R + 1]) {
    if (R == 2) {
        float g1[5];
        const float sum = usm_gauss(p[0], g1);
#pragma unroll
        for (int i = 0; i < 5; ++i) g1[i] = g1[i] / sum;
#pragma unroll
        for (int i = 0; i < 2 * R + 1; ++i)
#pragma unroll
            for (int j = 0; j < 2 * R + 1; ++j) w[i][j] = g1[i] * g1[j];
        return p[1];
    }
    const float a = 1.0f / 13.0f, c5 = 5.0f / 13.0f;
#pragma unroll
    for (int i = 0; i < 2 * R + 1; ++i)
#pragma unroll
        for (int j = 0; j < 2 * R + 1; ++j) w[i][j] = (i == R && j == R) ? c5 : a;
    return p[0];
}

}  // namespace adaisp
