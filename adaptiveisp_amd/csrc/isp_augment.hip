// Training augmentation of the replay-pool input (include/adaisp.h, adaisp_augment_u8): decoded uint8 HWC BGR images,
// each letterboxed at (top, left) of an S x S frame -> one uint8 HWC BGR S x S frame per image: an affine warp of the
// letterboxed frame (random_perspective with perspective = 0, augmentations.py:144-193, and the two flips of
// dataset.py:505-514 folded into the map), then the HSV tables of augment_hsv (augmentations.py:67-80). It runs BEFORE
// adaisp_unprocess / adaisp_unprocess_bayer: the sensor model sees the warped 8-bit scene, so its noise stays white.
//
// Everything is integer arithmetic; a numpy int64 restatement (tests/_augref.py) matches it bit for bit.
//
// Warp, for output pixel (x, y) and the image's inverse map m[0..5] (Q16, int64; sums wrap modulo 2^64):
//     fx = m0 * x + m1 * y + m2            fy = m3 * x + m4 * y + m5
//     X = fx >> 16, Y = fy >> 16           (arithmetic shift: floor)
//     ax = (fx >> 11) & 31, ay = (fy >> 11) & 31                               (weights in 1/32 pixel)
//     P(i, j) = the source pixel at row j - top, column i - left when that lies in [0, h) x [0, w), else `fill`;
//               each of the four taps on its own
//     v = ((32 - ax) (32 - ay) P(X, Y) + ax (32 - ay) P(X + 1, Y) + (32 - ax) ay P(X, Y + 1) + ax ay P(X + 1, Y + 1)
//          + 512) >> 10                                                        per channel
// Coordinates are pixel indices without a half-pixel shift (cv2.warpAffine's convention). With the identity map
// (m = 65536, 0, 0, 0, 65536, 0) ax = ay = 0 and v = P(x, y): the letterboxed frame, byte for byte.
//
// Colour, when the image has a table (lut >= 0), on the warped 8-bit (b, g, r); every `/` is a division of
// non-negative integers rounded down, so (2 n + d) / (2 d) is n / d rounded to nearest, halves up:
//   BGR -> HSV (cv2.COLOR_BGR2HSV's 8-bit ranges: H in [0, 180), S and V in [0, 255]):
//     V = max(b, g, r), d = V - min(b, g, r)
//     S = 0 when V = 0, else (255 d + V / 2) / V
//     H = 0 when d = 0; else with
//         n = 30 (g - b), plus 180 d when that is negative      when V = r
//         n = 30 (b - r) + 60 d                                 else when V = g
//         n = 30 (r - g) + 120 d                                else
//     H = (2 n + d) / (2 d), and 180 becomes 0
//   tables: H' = T[H], S' = T[256 + S], V' = T[512 + V] (768 bytes per image), then H' = H' mod 180
//   HSV -> BGR: i = H' / 30, f = H' - 30 i,
//     p = (V' (255 - S') + 127) / 255
//     q = (V' (7650 - S' f) + 3825) / 7650
//     t = (V' (7650 - S' (30 - f)) + 3825) / 7650
//     (r, g, b) = (V', t, p), (q, V', p), (p, V', t), (p, q, V'), (t, p, V'), (V', p, q)   for i = 0 .. 5
//
// Mapping from the output side: a lane owns 4 consecutive pixels of one output row (12 bytes: three dword stores when
// S % 4 == 0 and `dst` is 4-byte aligned, byte stores otherwise) and gathers its <= 16 source pixels with byte loads,
// so an image may start at any byte offset of `src`; a batch's sources are a few MB and stay in the L2. The image's
// table is copied into LDS once per workgroup (768 bytes, the only LDS).
#include "isp_internal.h"

static_assert(sizeof(adaisp_augment_desc) == 80, "adaisp_augment_desc is 80 bytes (adaptiveisp_amd/_lib.py)");

namespace adaisp {
namespace {

constexpr int AUG_THREADS = 256;

struct Bgr {
    unsigned b, g, r;
};

__device__ __forceinline__ unsigned umin3(unsigned a, unsigned b, unsigned c) { return min(a, min(b, c)); }
__device__ __forceinline__ unsigned umax3(unsigned a, unsigned b, unsigned c) { return max(a, max(b, c)); }

// the header comment's BGR -> HSV -> tables -> BGR
__device__ __forceinline__ Bgr hsv_tables(Bgr c, const uint8_t* lut) {
    const unsigned V = umax3(c.b, c.g, c.r), d = V - umin3(c.b, c.g, c.r);
    const unsigned S = V ? (255u * d + (V >> 1)) / V : 0u;
    unsigned H = 0;
    if (d) {
        int n;
        if (V == c.r) {
            n = 30 * ((int)c.g - (int)c.b);
            if (n < 0) n += 180 * (int)d;
        } else if (V == c.g) {
            n = 30 * ((int)c.b - (int)c.r) + 60 * (int)d;
        } else {
            n = 30 * ((int)c.r - (int)c.g) + 120 * (int)d;
        }
        H = (2u * (unsigned)n + d) / (2u * d);
        if (H >= 180u) H -= 180u;
    }
    const unsigned h = lut[H] % 180u, s = lut[256 + S], v = lut[512 + V];
    const unsigned i = h / 30u, f = h - 30u * i;
    const unsigned p = (v * (255u - s) + 127u) / 255u;
    const unsigned q = (v * (7650u - s * f) + 3825u) / 7650u;
    const unsigned t = (v * (7650u - s * (30u - f)) + 3825u) / 7650u;
    Bgr o;
    o.r = (i == 0 || i == 5) ? v : (i == 1) ? q : (i == 4) ? t : p;
    o.g = (i == 1 || i == 2) ? v : (i == 0) ? t : (i == 3) ? q : p;
    o.b = (i == 3 || i == 4) ? v : (i == 2) ? t : (i == 5) ? q : p;
    return o;
}

template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void k_augment_u8(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const adaisp_augment_desc* __restrict__ desc,
                                                            const uint8_t* __restrict__ luts, int n_luts,
                                                            uint8_t* __restrict__ dst, int S, int quads_per_row,
                                                            unsigned fill) {
    const int b = blockIdx.y;
    const adaisp_augment_desc& d = desc[b];
    __shared__ uint8_t lut[768];
    const bool colour = d.lut >= 0 && d.lut < n_luts;        // uniform over the workgroup; a table outside `luts`: none
    if (colour) {
        const uint8_t* __restrict__ t = luts + (int64_t)d.lut * 768;
#pragma unroll
        for (int k = 0; k < 3; ++k) lut[k * AUG_THREADS + threadIdx.x] = t[k * AUG_THREADS + threadIdx.x];
        __syncthreads();
    }
    const long q = (long)blockIdx.x * AUG_THREADS + threadIdx.x;
    if (q >= (long)S * quads_per_row) return;
    const int y = (int)(q / quads_per_row), x0 = (int)(q - (long)y * quads_per_row) * 4;
    const int h = d.h, w = d.w, top = d.top, left = d.left;
    // a placement that does not fit the S x S frame, or pixels that do not lie inside src, are never read: all fill
    const bool fits = h >= 0 && w >= 0 && top >= 0 && left >= 0 && top <= S - h && left <= S - w && d.src_offset >= 0 &&
                      d.src_offset <= src_bytes - (int64_t)h * w * 3;
    const uint8_t* __restrict__ img = src + (fits ? d.src_offset : 0);
    const Bgr pad = {fill & 255u, (fill >> 8) & 255u, (fill >> 16) & 255u};
    // unsigned sums: the wrap modulo 2^64 is defined, and is numpy's
    const uint64_t m0 = (uint64_t)d.m[0], m3 = (uint64_t)d.m[3];
    uint64_t fx = m0 * (uint64_t)x0 + (uint64_t)d.m[1] * (uint64_t)y + (uint64_t)d.m[2];
    uint64_t fy = m3 * (uint64_t)x0 + (uint64_t)d.m[4] * (uint64_t)y + (uint64_t)d.m[5];

    auto tap = [&](int64_t i, int64_t j) {
        const int64_t ix = i - left, iy = j - top;
        if (!fits || ix < 0 || ix >= w || iy < 0 || iy >= h) return pad;
        const uint8_t* __restrict__ px = img + (iy * w + ix) * 3;
        return Bgr{px[0], px[1], px[2]};
    };

    uint8_t o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k, fx += m0, fy += m3) {
        const int64_t X = (int64_t)fx >> 16, Y = (int64_t)fy >> 16;
        const unsigned ax = (unsigned)((int64_t)fx >> 11) & 31u, ay = (unsigned)((int64_t)fy >> 11) & 31u;
        const Bgr p00 = tap(X, Y), p10 = tap(X + 1, Y), p01 = tap(X, Y + 1), p11 = tap(X + 1, Y + 1);
        const unsigned w00 = (32u - ax) * (32u - ay), w10 = ax * (32u - ay), w01 = (32u - ax) * ay, w11 = ax * ay;
        Bgr v;
        v.b = (w00 * p00.b + w10 * p10.b + w01 * p01.b + w11 * p11.b + 512u) >> 10;
        v.g = (w00 * p00.g + w10 * p10.g + w01 * p01.g + w11 * p11.g + 512u) >> 10;
        v.r = (w00 * p00.r + w10 * p10.r + w01 * p01.r + w11 * p11.r + 512u) >> 10;
        if (colour) v = hsv_tables(v, lut);
        o[3 * k] = (uint8_t)v.b;
        o[3 * k + 1] = (uint8_t)v.g;
        o[3 * k + 2] = (uint8_t)v.r;
    }
    uint8_t* __restrict__ out = dst + ((long)b * S * S + (long)y * S + x0) * 3;
    if (VEC) {
        uint32_t* __restrict__ out4 = reinterpret_cast<uint32_t*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            out4[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) |
                      ((uint32_t)o[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + k < S) {
                out[3 * k] = o[3 * k];
                out[3 * k + 1] = o[3 * k + 1];
                out[3 * k + 2] = o[3 * k + 2];
            }
        }
    }
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_augment_u8(const uint8_t* src, size_t src_bytes, const adaisp_augment_desc* desc,
                                 const uint8_t* luts, int n_luts, uint8_t* dst, int B, int S, unsigned fill,
                                 void* stream) {
    using namespace adaisp;
    if (!src || !desc || !dst || B < 1 || S < 1 || n_luts < 0 || (!luts && n_luts > 0)) return ADAISP_EINVAL;
    if (fill > 0xFFFFFFu || src_bytes > (size_t)INT64_MAX) return ADAISP_EINVAL;
    if (B > 65535 || S > 32768) return ADAISP_ESHAPE;              // grid.y; pixel indices fit 32 bits
    const int qpr = (S + 3) / 4;
    const long quads = (long)S * qpr;
    const dim3 grid((unsigned)((quads + AUG_THREADS - 1) / AUG_THREADS), (unsigned)B);
    const bool vec = (S % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 4 == 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL((k_augment_u8<true>), grid, dim3(AUG_THREADS), 0, s, src, (int64_t)src_bytes, desc, luts, n_luts,
                           dst, S, qpr, fill);
    else
        hipLaunchKernelGGL((k_augment_u8<false>), grid, dim3(AUG_THREADS), 0, s, src, (int64_t)src_bytes, desc, luts,
                           n_luts, dst, S, qpr, fill);
    return hipGetLastError() == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
