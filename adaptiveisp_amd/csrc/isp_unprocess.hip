// Replay-pool input conversion (include/adaisp.h, adaisp_unprocess): decoded uint8 HWC BGR images -> planar fp32
// [B,3,S,S] RGB, letterboxed in place (every sample outside an image's (h, w, top, left) rectangle is exactly 0).
//
//   convert (flags 0):   out = float(u8) / 255                            the `lod` loader, dataset.py:794-897
//   ADAISP_UNP_UNPROCESS: unprocess_wo_mosaic in fp32                     isp/unprocess_np.py:248-292
//       x = rgb * prescale;  x = 0.5 - sin(asin(1 - 2 clip(x)) / 3);  x = max(x, 1e-8)^2.2   (a 256-entry table per
//       image, built in LDS by each workgroup: it depends on the 8-bit value alone);  x = rgb2cam x;
//       gray = mean(x);  mask = (max(gray - 0.9, 0) / 0.1)^2;  x *= max(mask + (1 - mask) g, g);  x = clip(x) * ratio
//   ADAISP_UNP_NOISE:    x = clip(x + N(0, 1) sqrt(x shot + read))         add_read_and_shot_noise, :177-181
//
// The reference pads AFTER the conversion (letterbox of the unprocessed image, dataset.py:458-475), so the pad gets no
// noise. The chain's device functions and the noise generator live in isp_unprocess_math.h, shared with the Bayer sensor
// (isp_sensor.hip).
//
// Mapping from the output side: a lane owns 4 consecutive samples of one output row and writes them to each plane as
// one 16-byte store (S % 4 == 0 and a 16-byte aligned `out`; scalar stores otherwise). It reads the <= 12 source bytes
// it needs with byte loads, so an image may start at any byte offset of `src`.
#include "isp_unprocess_math.h"

static_assert(sizeof(adaisp_unprocess_desc) == 96, "adaisp_unprocess_desc is 96 bytes (adaptiveisp_amd/_lib.py)");

namespace adaisp {
namespace {

constexpr int UNP_THREADS = 256;   // = the 256 entries of the per-image tone table

template <int MODE, bool VEC>   // MODE: 0 convert, 1 unprocess, 2 unprocess + noise
__global__ __launch_bounds__(UNP_THREADS) void k_unprocess(const uint8_t* __restrict__ src,
                                                           const adaisp_unprocess_desc* __restrict__ desc,
                                                           float* __restrict__ out, int S, int quads_per_row,
                                                           uint64_t seed) {
    const int b = blockIdx.y;
    const adaisp_unprocess_desc& d = desc[b];
    // the tone curve and gamma depend on the 8-bit value alone: one table of 256 per image (and workgroup) instead of
    // three asin / sin / pow per pixel
    __shared__ float lut[256];
    if (MODE > 0) {
        lut[threadIdx.x] = tone_gamma(threadIdx.x, d.p[ADAISP_UNP_PRESCALE]);
        __syncthreads();
    }
    const long q = (long)blockIdx.x * UNP_THREADS + threadIdx.x;
    if (q >= (long)S * quads_per_row) return;
    const int y = (int)(q / quads_per_row), x0 = (int)(q - (long)y * quads_per_row) * 4;
    const int h = d.h, w = d.w, top = d.top, left = d.left;
    // a placement that does not fit the S x S frame is never read from: the image comes out all zero
    const bool fits = h >= 0 && w >= 0 && top >= 0 && left >= 0 && top <= S - h && left <= S - w;
    const int iy = y - top;
    const bool row_in = fits && iy >= 0 && iy < h;
    const uint8_t* __restrict__ row = src + d.src_offset + (long)iy * w * 3;
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = x0 + k - left;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (row_in && ix >= 0 && ix < w && x0 + k < S) {
            const uint8_t* __restrict__ px = row + ix * 3;                           // BGR
            if (MODE > 0) {
                const float t[3] = {lut[px[2]], lut[px[1]], lut[px[0]]};
                unprocess_px<MODE == 2>(t, v, d.p, seed, d.serial, (uint32_t)(iy * w + ix));
            } else {
                v[0] = (float)px[2] / 255.0f;
                v[1] = (float)px[1] / 255.0f;
                v[2] = (float)px[0] / 255.0f;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][k] = v[c];
    }
    const long plane = (long)S * S;
    float* __restrict__ dst = out + (long)b * 3 * plane + (long)y * S + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC) {
            *reinterpret_cast<float4*>(dst + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < S) dst[c * plane + k] = o[c][k];
        }
    }
}

template <int MODE>
hipError_t launch_mode(const uint8_t* src, const adaisp_unprocess_desc* desc, float* out, int B, int S, uint64_t seed,
                       hipStream_t s) {
    const int qpr = (S + 3) / 4;
    const long quads = (long)S * qpr;
    const dim3 grid((unsigned)((quads + UNP_THREADS - 1) / UNP_THREADS), (unsigned)B);
    const bool vec = (S % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    if (vec)
        hipLaunchKernelGGL((k_unprocess<MODE, true>), grid, dim3(UNP_THREADS), 0, s, src, desc, out, S, qpr, seed);
    else
        hipLaunchKernelGGL((k_unprocess<MODE, false>), grid, dim3(UNP_THREADS), 0, s, src, desc, out, S, qpr, seed);
    return hipGetLastError();
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_unprocess(const uint8_t* src, const adaisp_unprocess_desc* desc, float* out, int B, int S,
                                uint64_t seed, unsigned flags, void* stream) {
    using namespace adaisp;
    if (!src || !desc || !out || B < 1 || S < 1) return ADAISP_EINVAL;
    if (flags & ~(ADAISP_UNP_UNPROCESS | ADAISP_UNP_NOISE)) return ADAISP_EINVAL;
    if ((flags & ADAISP_UNP_NOISE) && !(flags & ADAISP_UNP_UNPROCESS)) return ADAISP_EINVAL;
    if (B > 65535 || S > 32768) return ADAISP_ESHAPE;              // grid.y; pixel indices and the counter fit 32 bits
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = (flags & ADAISP_UNP_NOISE) ? launch_mode<2>(src, desc, out, B, S, seed, s)
                         : (flags & ADAISP_UNP_UNPROCESS) ? launch_mode<1>(src, desc, out, B, S, seed, s)
                                                          : launch_mode<0>(src, desc, out, B, S, seed, s);
    return e == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
