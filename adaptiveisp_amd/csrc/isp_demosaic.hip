// Bayer demosaic front-end — an EXTENSION: the reference's ISP starts from a 3-channel linear
// image and has no demosaic; only the inverse packing exists (`mosaic`, isp/unprocess_np.py:82-98,
// `reconstruct_bayer` :111-128). north_star asks for a raw-Bayer entry to the path, so this kernel is defined by its
// own oracle (oracle_demosaic in oracle/isp_oracle.c) and checked for consistency with that packing.
//
// raw: uint16 [B,H,W], one colour sample per pixel (pattern gives the position of the red sample in the 2x2 cell);
// out: planar fp32 [B,3,H,W] = bilinear interpolation of the normalised samples s = (raw - black) * 1/(white - black):
//   at a sampled colour: the sample;  green at red/blue sites: ((N + S) + (W + E)) / 4;
//   red/blue at green sites: (W + E) / 2 or (N + S) / 2;  red at blue sites (and v.v.): ((NW + NE) + (SW + SE)) / 4;
// image borders mirror without repeating the edge sample (index -1 -> 1, H -> H-2), which preserves the Bayer phase.
//
// Memory-bound: 2 B/px in, 12 B/px out. One workgroup = a 128 x 32 pixel tile: the tile plus a one-pixel ring is
// staged in LDS as fp32 samples (34 x 130), then each lane produces 2x2 cells — two adjacent pixels per row, so every
// plane is written with 8-byte stores, 512 contiguous bytes per wave and row.
#include "isp_internal.h"
#include "isp_demosaic_math.h"

namespace adaisp {
namespace {

constexpr int TW = 128, TH = 32, LW = TW + 2, LH = TH + 2;

// mirror(), reflect2() and the per-site math: isp_demosaic_math.h (shared with isp_raw_load.hip)

__global__ __launch_bounds__(256) void k_demosaic(const unsigned short* __restrict__ raw, float* __restrict__ out,
                                                  int H, int W, int ry, int rx, float black, float inv_range) {
    __shared__ float s[LH][LW + 2];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const unsigned short* __restrict__ src = raw + (long)b * H * W;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int y = mirror(y0 + ly - 1, H), x = mirror(x0 + lx - 1, W);
        s[ly][lx] = ((float)src[(long)y * W + x] - black) * inv_range;
    }
    __syncthreads();
    const long plane = (long)H * W;
    float* __restrict__ o = out + (long)b * 3 * plane;
    // 64 x 16 cells per tile, 4 per thread: thread -> cell column (tid & 63), cell rows (tid >> 6) + 4*k
    const int cx = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cy = (threadIdx.x >> 6) + 4 * k;
        const int gx = x0 + 2 * cx, gy = y0 + 2 * cy;
        if (gx >= W || gy >= H) continue;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            float r[2], g[2], bl[2];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ly = 2 * cy + dy + 1, lx = 2 * cx + dx + 1;
                const float c = s[ly][lx];
                const float n = s[ly - 1][lx], so = s[ly + 1][lx], w = s[ly][lx - 1], e = s[ly][lx + 1];
                bilinear_site(c, n, so, w, e, s[ly - 1][lx - 1], s[ly - 1][lx + 1], s[ly + 1][lx - 1], s[ly + 1][lx + 1],
                              (gy + dy - ry) & 1, (gx + dx - rx) & 1, r[dx], g[dx], bl[dx]);
            }
            const long off = (long)(gy + dy) * W + gx;
            *reinterpret_cast<float2*>(o + off) = make_float2(r[0], r[1]);
            *reinterpret_cast<float2*>(o + plane + off) = make_float2(g[0], g[1]);
            *reinterpret_cast<float2*>(o + 2 * plane + off) = make_float2(bl[0], bl[1]);
        }
    }
}

// The same rule inside every image's own rectangle of a letterboxed S x S frame (adaisp_demosaic_rects): the plane of
// adaisp_unprocess_bayer holds image b at (top, left), h x w, and black around it. The CFA phase and the mirror belong to
// the rectangle (iy = y - top, ix = x - left; -1 -> 1, h -> h - 2), so a border pixel never averages with the pad and an
// odd top / left keeps the colours in place; every output outside the rectangle is exactly 0. The tile grid covers the
// frame; the staging reads through the rectangle's mirror, so a tile's ring comes from inside the image whatever lies
// beside it. A tile that misses the rectangle stages nothing and writes zeros. Cells are aligned to the frame: 8-byte
// stores when S is even and `out` 8-byte aligned (VEC), one store per sample otherwise.
template <bool VEC>
__global__ __launch_bounds__(256) void k_demosaic_rects(const unsigned short* __restrict__ raw,
                                                        const adaisp_unprocess_desc* __restrict__ desc,
                                                        float* __restrict__ out, int S, int ry, int rx, float black,
                                                        float inv_range) {
    __shared__ float s[LH][LW + 2];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const adaisp_unprocess_desc& d = desc[b];
    const int h = d.h, w = d.w, top = d.top, left = d.left;
    // as adaisp_unprocess_bayer: a placement that does not fit the frame is never read from; an image without a second
    // row or column has nothing to mirror onto and comes out all zero
    const bool fits = h >= 2 && w >= 2 && top >= 0 && left >= 0 && top <= S - h && left <= S - w;
    const bool hit = fits && y0 < top + h && y0 + TH > top && x0 < left + w && x0 + TW > left;   // workgroup-uniform
    const long plane = (long)S * S;
    if (hit) {
        const unsigned short* __restrict__ src = raw + (long)b * plane + (long)top * S + left;
        for (int i = threadIdx.x; i < LH * LW; i += 256) {
            const int ly = i / LW, lx = i - ly * LW;
            const int y = mirror(y0 + ly - 1 - top, h), x = mirror(x0 + lx - 1 - left, w);
            s[ly][lx] = ((float)src[(long)y * S + x] - black) * inv_range;
        }
        __syncthreads();
    }
    float* __restrict__ o = out + (long)b * 3 * plane;
    const int cx = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cy = (threadIdx.x >> 6) + 4 * k;
        const int gx = x0 + 2 * cx, gy = y0 + 2 * cy;
        if (gx >= S || gy >= S) continue;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            float r[2], g[2], bl[2];
            const int iy = gy + dy - top;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = gx + dx - left;
                r[dx] = g[dx] = bl[dx] = 0.0f;
                if (!hit || iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
                const int ly = 2 * cy + dy + 1, lx = 2 * cx + dx + 1;
                const float c = s[ly][lx];
                const float n = s[ly - 1][lx], so = s[ly + 1][lx], we = s[ly][lx - 1], e = s[ly][lx + 1];
                bilinear_site(c, n, so, we, e, s[ly - 1][lx - 1], s[ly - 1][lx + 1], s[ly + 1][lx - 1], s[ly + 1][lx + 1],
                              (iy - ry) & 1, (ix - rx) & 1, r[dx], g[dx], bl[dx]);
            }
            if (gy + dy >= S) continue;                                          // odd S: the last cell row is half a cell
            const long off = (long)(gy + dy) * S + gx;
            if (VEC) {
                *reinterpret_cast<float2*>(o + off) = make_float2(r[0], r[1]);
                *reinterpret_cast<float2*>(o + plane + off) = make_float2(g[0], g[1]);
                *reinterpret_cast<float2*>(o + 2 * plane + off) = make_float2(bl[0], bl[1]);
            } else {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
                    if (gx + dx < S) {
                        o[off + dx] = r[dx];
                        o[plane + off + dx] = g[dx];
                        o[2 * plane + off + dx] = bl[dx];
                    }
            }
        }
    }
}

// Gradient-corrected interpolation (Malvar, He, Cutler 2004; adaisp_demosaic_ex / adaisp_demosaic_rects_ex with
// ADAISP_DEMOSAIC_MHC): the 5 x 5 linear filters of include/adaisp.h on the UN-normalised samples t = float(raw) - black,
//   the site's own colour                8C
//   green at a red / blue site           4C + 2(N + S + W + E) - (N2 + S2 + W2 + E2)
//   red at a blue site (and v.v.)        6C + 2D - 1.5(N2 + S2 + W2 + E2),  D = NW + NE + SW + SE
//   red / blue at a green site, W / E    5C + 4(W + E) - D - (W2 + E2) + 0.5(N2 + S2)
//   red / blue at a green site, N / S    5C + 4(N + S) - D - (N2 + S2) + 0.5(W2 + E2)
// and out = (acc * 0.125f) * inv_range.
// Every term is a multiple of 0.5 and 2|acc| <= 40 * 65535 < 2^24 for whole-number levels, so acc is exact in fp32 in any
// order and under FMA contraction: the one rounding is the last multiply, and a sampled colour is bit for bit the bilinear
// kernels' (raw - black) * inv_range. Nothing is clamped: the filters overshoot at edges and the filter stack clips.
//
// Same tile as above with a two-pixel ring: 36 x 132 fp32 in LDS. The row stride is the staged width itself, 132: the
// staging index IS the LDS address (consecutive lanes, consecutive banks), and 132 is even, so a lane's six samples of a
// row, starting at the even column 2 cx, are three aligned 8-byte reads; a wave reads one row at a time (all 64 cell
// columns of it), 64 consecutive dwords per half-wave, so neither the row taps nor the column taps (which are other rows,
// read by the same lane) meet a bank twice. Unlike above a wave owns four cell rows that ADJOIN (pixel rows 8 wave ..
// 8 wave + 7): their 6-row windows overlap, 12 LDS rows serve what 24 would, and a store is still 512 contiguous bytes
// per wave and row.
constexpr int MR = 2, MLW = TW + 2 * MR, MLH = TH + 2 * MR;

// One lane's 12 x 6 window: LDS rows 8 wave .. 8 wave + 11, columns 2 cx .. 2 cx + 5; pixel (8 wave + j, 2 cx + i) of the
// tile is v[j + 2][i + 2].
__device__ __forceinline__ void mhc_window(const float (&s)[MLH][MLW], int wave, int cx, float (&v)[12][6]) {
#pragma unroll
    for (int j = 0; j < 12; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float2 p = *reinterpret_cast<const float2*>(&s[8 * wave + j][2 * cx + 2 * i]);
            v[j][2 * i] = p.x;
            v[j][2 * i + 1] = p.y;
        }
}

// The three colours at v[y][x], a site of phase (py, px): 0,0 = red site; 1,1 = blue site; py, px are wave-uniform.
__device__ __forceinline__ void mhc_site(const float (&v)[12][6], int y, int x, int py, int px, float inv_range,
                                         float& r, float& g, float& b) {
    const float c = v[y][x];
    const float a1h = v[y][x - 1] + v[y][x + 1], a1v = v[y - 1][x] + v[y + 1][x];
    const float a2h = v[y][x - 2] + v[y][x + 2], a2v = v[y - 2][x] + v[y + 2][x];
    const float d = (v[y - 1][x - 1] + v[y - 1][x + 1]) + (v[y + 1][x - 1] + v[y + 1][x + 1]);
    mhc_site_sums(c, a1h, a1v, a2h, a2v, d, py, px, inv_range, r, g, b);
}

__global__ __launch_bounds__(256) void k_demosaic_mhc(const unsigned short* __restrict__ raw, float* __restrict__ out,
                                                      int H, int W, int ry, int rx, float black, float inv_range) {
    __shared__ __attribute__((aligned(8))) float s[MLH][MLW];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const unsigned short* __restrict__ src = raw + (long)b * H * W;
    for (int i = threadIdx.x; i < MLH * MLW; i += 256) {
        const int ly = i / MLW, lx = i - ly * MLW;
        const int y = reflect2(y0 + ly - MR, H), x = reflect2(x0 + lx - MR, W);
        (&s[0][0])[i] = (float)src[(long)y * W + x] - black;
    }
    __syncthreads();
    const long plane = (long)H * W;
    float* __restrict__ o = out + (long)b * 3 * plane;
    // 64 x 16 cells per tile, 4 per thread: thread -> cell column (tid & 63), cell rows 4 * (tid >> 6) + k
    const int cx = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx = x0 + 2 * cx;
    if (gx >= W || y0 + 8 * wave >= H) return;
    float v[12][6];
    mhc_window(s, wave, cx, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int gy = y0 + 8 * wave + 2 * k;
        if (gy >= H) break;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            float r[2], g[2], bl[2];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
                mhc_site(v, 2 * k + dy + 2, dx + 2, (dy - ry) & 1, (dx - rx) & 1, inv_range, r[dx], g[dx], bl[dx]);
            const long off = (long)(gy + dy) * W + gx;
            *reinterpret_cast<float2*>(o + off) = make_float2(r[0], r[1]);
            *reinterpret_cast<float2*>(o + plane + off) = make_float2(g[0], g[1]);
            *reinterpret_cast<float2*>(o + 2 * plane + off) = make_float2(bl[0], bl[1]);
        }
    }
}

// k_demosaic_rects' contract with the filters above: phase and reflection belong to the rectangle (iy = y - top,
// ix = x - left), zeros outside it, an image with a side under 2 or a placement that does not fit all zero, a tile that
// misses the rectangle stages nothing. Inside a tile that hits, every LDS sample is staged (through the reflection and its
// clamp), so the filters run on all cells and the rectangle test only selects between their result and 0.
template <bool VEC>
__global__ __launch_bounds__(256) void k_demosaic_mhc_rects(const unsigned short* __restrict__ raw,
                                                            const adaisp_unprocess_desc* __restrict__ desc,
                                                            float* __restrict__ out, int S, int ry, int rx, float black,
                                                            float inv_range) {
    __shared__ __attribute__((aligned(8))) float s[MLH][MLW];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const adaisp_unprocess_desc& d = desc[b];
    const int h = d.h, w = d.w, top = d.top, left = d.left;
    const bool fits = h >= 2 && w >= 2 && top >= 0 && left >= 0 && top <= S - h && left <= S - w;
    const bool hit = fits && y0 < top + h && y0 + TH > top && x0 < left + w && x0 + TW > left;   // workgroup-uniform
    const long plane = (long)S * S;
    if (hit) {
        const unsigned short* __restrict__ src = raw + (long)b * plane + (long)top * S + left;
        for (int i = threadIdx.x; i < MLH * MLW; i += 256) {
            const int ly = i / MLW, lx = i - ly * MLW;
            const int y = reflect2(y0 + ly - MR - top, h), x = reflect2(x0 + lx - MR - left, w);
            (&s[0][0])[i] = (float)src[(long)y * S + x] - black;
        }
        __syncthreads();
    }
    float* __restrict__ o = out + (long)b * 3 * plane;
    const int cx = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx = x0 + 2 * cx;
    if (gx >= S || y0 + 8 * wave >= S) return;
    float v[12][6];
    if (hit) mhc_window(s, wave, cx, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int gy = y0 + 8 * wave + 2 * k;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            if (gy + dy >= S) break;                                             // odd S: the last cell row is half a cell
            float r[2], g[2], bl[2];
            const int iy = gy + dy - top;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = gx + dx - left;
                r[dx] = g[dx] = bl[dx] = 0.0f;
                if (!hit) continue;
                float fr, fg, fb;
                mhc_site(v, 2 * k + dy + 2, dx + 2, (iy - ry) & 1, (ix - rx) & 1, inv_range, fr, fg, fb);
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) { r[dx] = fr; g[dx] = fg; bl[dx] = fb; }
            }
            const long off = (long)(gy + dy) * S + gx;
            if (VEC) {
                *reinterpret_cast<float2*>(o + off) = make_float2(r[0], r[1]);
                *reinterpret_cast<float2*>(o + plane + off) = make_float2(g[0], g[1]);
                *reinterpret_cast<float2*>(o + 2 * plane + off) = make_float2(bl[0], bl[1]);
            } else {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
                    if (gx + dx < S) {
                        o[off + dx] = r[dx];
                        o[plane + off + dx] = g[dx];
                        o[2 * plane + off + dx] = bl[dx];
                    }
            }
        }
    }
}

}  // namespace

hipError_t launch_demosaic_rects(const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int S,
                                 int pattern, float black, float white, hipStream_t s) {
    const int ry = pattern >> 1, rx = pattern & 1;
    dim3 grid((S + TW - 1) / TW, (S + TH - 1) / TH, B);
    const float inv = 1.0f / (white - black);
    if (S % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0)
        hipLaunchKernelGGL((k_demosaic_rects<true>), grid, dim3(256), 0, s, raw, desc, out, S, ry, rx, black, inv);
    else
        hipLaunchKernelGGL((k_demosaic_rects<false>), grid, dim3(256), 0, s, raw, desc, out, S, ry, rx, black, inv);
    return hipGetLastError();
}

hipError_t launch_demosaic_mhc_rects(const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int S,
                                     int pattern, float black, float white, hipStream_t s) {
    const int ry = pattern >> 1, rx = pattern & 1;
    dim3 grid((S + TW - 1) / TW, (S + TH - 1) / TH, B);
    const float inv = 1.0f / (white - black);
    if (S % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0)
        hipLaunchKernelGGL((k_demosaic_mhc_rects<true>), grid, dim3(256), 0, s, raw, desc, out, S, ry, rx, black, inv);
    else
        hipLaunchKernelGGL((k_demosaic_mhc_rects<false>), grid, dim3(256), 0, s, raw, desc, out, S, ry, rx, black, inv);
    return hipGetLastError();
}

hipError_t launch_demosaic_mhc(const uint16_t* raw, float* out, int B, int H, int W, int pattern, float black, float white,
                               hipStream_t s) {
    const int ry = pattern >> 1, rx = pattern & 1;
    dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
    hipLaunchKernelGGL(k_demosaic_mhc, grid, dim3(256), 0, s, raw, out, H, W, ry, rx, black, 1.0f / (white - black));
    return hipGetLastError();
}

hipError_t launch_demosaic(const uint16_t* raw, float* out, int B, int H, int W, int pattern, float black, float white,
                           hipStream_t s) {
    const int ry = pattern >> 1, rx = pattern & 1;
    dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
    hipLaunchKernelGGL(k_demosaic, grid, dim3(256), 0, s, raw, out, H, W, ry, rx, black, 1.0f / (white - black));
    return hipGetLastError();
}

}  // namespace adaisp
