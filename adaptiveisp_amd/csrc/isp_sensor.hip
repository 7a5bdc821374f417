// Simulated Bayer sensor (include/adaisp.h, adaisp_unprocess_bayer): decoded uint8 HWC BGR images -> one uint16
// colour-filter-array plane [B,S,S], letterboxed in place. The reference's `unprocess` ends in `mosaic`
// (isp/unprocess_np.py:217-245, :82-98): every pixel keeps one channel of the unprocessed image, the colour its filter
// passes, and a camera adds its noise to that one measurement. So pixel (iy, ix) of an image, in the image's own
// coordinates, keeps channel c of the CFA cell (red at (ry, rx) = (pattern >> 1, pattern & 1), blue diagonally across,
// green elsewhere), and
//
//   v      = the fp32 value adaisp_unprocess writes for channel c of that pixel under the same flags, parameters, seed and
//            serial (convert, unprocess, unprocess + noise: isp_unprocess_math.h builds both kernels' pixels; with noise, v
//            carries the c-th of the pixel's three normals, so it IS the three-channel kernel's noisy channel)
//   sample = clamp(rintf(v * (white - black)) + black, 0, 65535)
//
// Every sample outside the image's (h, w, top, left) rectangle is `black`: the pad is a dark sensor, not a negative one.
// The kernel computes what the kept channel needs: the three rows of the colour matrix (the saturation mask takes their
// mean), then one gain, one clip, one Box-Muller pair.
//
// Memory-bound, 3 B/px in and 2 B/px out. Mapping from the output side, as k_unprocess: a lane owns 4 consecutive samples
// of one output row and writes them as one 8-byte store (S % 4 == 0 and an 8-byte aligned `out`; one 2-byte store per
// sample otherwise). It reads the <= 12 source bytes it needs with byte loads, so an image may start at any byte offset.
#include "isp_unprocess_math.h"

namespace adaisp {
namespace {

constexpr int SENSOR_THREADS = 256;   // = the 256 entries of the per-image tone table

__device__ __forceinline__ unsigned short quantise(float v, float range, float black) {
    return (unsigned short)fminf(fmaxf(rintf(v * range) + black, 0.0f), 65535.0f);
}

template <int MODE, bool VEC>   // MODE: 0 convert, 1 unprocess, 2 unprocess + noise
__global__ __launch_bounds__(SENSOR_THREADS) void k_unprocess_bayer(const uint8_t* __restrict__ src,
                                                                    const adaisp_unprocess_desc* __restrict__ desc,
                                                                    unsigned short* __restrict__ out, int S,
                                                                    int quads_per_row, uint64_t seed, int ry, int rx,
                                                                    float black, float range) {
    const int b = blockIdx.y;
    const adaisp_unprocess_desc& d = desc[b];
    __shared__ float lut[256];
    if (MODE > 0) {
        lut[threadIdx.x] = tone_gamma(threadIdx.x, d.p[ADAISP_UNP_PRESCALE]);
        __syncthreads();
    }
    const long q = (long)blockIdx.x * SENSOR_THREADS + threadIdx.x;
    if (q >= (long)S * quads_per_row) return;
    const int y = (int)(q / quads_per_row), x0 = (int)(q - (long)y * quads_per_row) * 4;
    const int h = d.h, w = d.w, top = d.top, left = d.left;
    // a placement that does not fit the S x S frame is never read from: the image comes out all black
    const bool fits = h >= 0 && w >= 0 && top >= 0 && left >= 0 && top <= S - h && left <= S - w;
    const int iy = y - top;
    const bool row_in = fits && iy >= 0 && iy < h;
    const uint8_t* __restrict__ row = src + d.src_offset + (long)iy * w * 3;
    const int py = (iy - ry) & 1;
    const unsigned short dark = quantise(0.0f, range, black);
    unsigned short o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = x0 + k - left;
        o[k] = dark;
        if (row_in && ix >= 0 && ix < w && x0 + k < S) {
            const int px = (ix - rx) & 1;
            const int c = py == px ? 2 * py : 1;                                     // 0,0 = red site; 1,1 = blue site
            const uint8_t* __restrict__ bgr = row + ix * 3;
            float v;
            if (MODE > 0) {
                const float t[3] = {lut[bgr[2]], lut[bgr[1]], lut[bgr[0]]};
                v = unprocess_ch<MODE == 2>(t, c, d.p, seed, d.serial, (uint32_t)(iy * w + ix));
            } else {
                v = (float)bgr[2 - c] / 255.0f;
            }
            o[k] = quantise(v, range, black);
        }
    }
    unsigned short* __restrict__ dst = out + (long)b * S * S + (long)y * S + x0;
    if (VEC) {
        *reinterpret_cast<ushort4*>(dst) = make_ushort4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < S) dst[k] = o[k];
    }
}

template <int MODE>
hipError_t launch_mode(const uint8_t* src, const adaisp_unprocess_desc* desc, uint16_t* out, int B, int S, uint64_t seed,
                       int pattern, float black, float white, hipStream_t s) {
    const int qpr = (S + 3) / 4;
    const long quads = (long)S * qpr;
    const dim3 grid((unsigned)((quads + SENSOR_THREADS - 1) / SENSOR_THREADS), (unsigned)B);
    const bool vec = (S % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 8 == 0);
    const int ry = pattern >> 1, rx = pattern & 1;
    if (vec)
        hipLaunchKernelGGL((k_unprocess_bayer<MODE, true>), grid, dim3(SENSOR_THREADS), 0, s, src, desc, out, S, qpr, seed,
                           ry, rx, black, white - black);
    else
        hipLaunchKernelGGL((k_unprocess_bayer<MODE, false>), grid, dim3(SENSOR_THREADS), 0, s, src, desc, out, S, qpr, seed,
                           ry, rx, black, white - black);
    return hipGetLastError();
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_unprocess_bayer(const uint8_t* src, const adaisp_unprocess_desc* desc, uint16_t* out, int B, int S,
                                      uint64_t seed, unsigned flags, int pattern, float black_level, float white_level,
                                      void* stream) {
    using namespace adaisp;
    if (!src || !desc || !out || B < 1 || S < 1) return ADAISP_EINVAL;
    if (flags & ~(ADAISP_UNP_UNPROCESS | ADAISP_UNP_NOISE)) return ADAISP_EINVAL;
    if ((flags & ADAISP_UNP_NOISE) && !(flags & ADAISP_UNP_UNPROCESS)) return ADAISP_EINVAL;
    if (pattern < 0 || pattern > 3 || !(white_level > black_level)) return ADAISP_EINVAL;
    if (B > 65535 || S > 32768) return ADAISP_ESHAPE;              // grid.y; pixel indices and the counter fit 32 bits
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e =
        (flags & ADAISP_UNP_NOISE) ? launch_mode<2>(src, desc, out, B, S, seed, pattern, black_level, white_level, s)
        : (flags & ADAISP_UNP_UNPROCESS) ? launch_mode<1>(src, desc, out, B, S, seed, pattern, black_level, white_level, s)
                                         : launch_mode<0>(src, desc, out, B, S, seed, pattern, black_level, white_level, s);
    return e == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
