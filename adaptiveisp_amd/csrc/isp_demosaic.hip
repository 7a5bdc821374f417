// Bayer demosaic front-end — an EXTENSION: the reference's ISP starts from a 3-channel linear
// image and has no demosaic; only the inverse packing exists (`mosaic`, isp/unprocess_np.py:82-98,
// `reconstruct_bayer` :111-128). north_star asks for a raw-Bayer entry to the path, so this kernel is defined by its
// own oracle (oracle_demosaic in oracle/isp_oracle.c) and checked for consistency with that packing.
//
// raw: uint16 [B,FH,FW], one colour sample per pixel (pattern gives the position of the red sample in the 2x2 cell);
// out: planar fp32 [B,3,FH,FW]. Two methods (isp_demosaic_math.h has the expressions), one kernel template:
//
// Bilinear, on the normalised samples s = (raw - black) * 1/(white - black):
//   at a sampled colour: the sample;  green at red/blue sites: ((N + S) + (W + E)) / 4;
//   red/blue at green sites: (W + E) / 2 or (N + S) / 2;  red at blue sites (and v.v.): ((NW + NE) + (SW + SE)) / 4.
//
// Gradient-corrected (Malvar, He, Cutler 2004; ADAISP_DEMOSAIC_MHC): the 5 x 5 linear filters of include/adaisp.h on the
// UN-normalised samples t = float(raw) - black,
//   the site's own colour                8C
//   green at a red / blue site           4C + 2(N + S + W + E) - (N2 + S2 + W2 + E2)
//   red at a blue site (and v.v.)        6C + 2D - 1.5(N2 + S2 + W2 + E2),  D = NW + NE + SW + SE
//   red / blue at a green site, W / E    5C + 4(W + E) - D - (W2 + E2) + 0.5(N2 + S2)
//   red / blue at a green site, N / S    5C + 4(N + S) - D - (N2 + S2) + 0.5(W2 + E2)
// and out = (acc * 0.125f) * inv_range.
// Every term is a multiple of 0.5 and 2|acc| <= 40 * 65535 < 2^24 for whole-number levels, so acc is exact in fp32 in any
// order and under FMA contraction: the one rounding is the last multiply, and a sampled colour is bit for bit the
// bilinear (raw - black) * inv_range. Nothing is clamped: the filters overshoot at edges and the filter stack clips.
//
// Borders reflect without repeating the edge sample (index -1 -> 1, n -> n - 2), which preserves the Bayer phase.
//
// Memory-bound: 2 B/px in, 12 B/px out. One workgroup = a 128 x 32 pixel tile: the tile plus the method's ring is staged
// in LDS as fp32 samples, then each lane produces 2x2 cells — two adjacent pixels per row, so every plane is written with
// 8-byte stores, 512 contiguous bytes per wave and row.
#include "isp_internal.h"
#include "isp_demosaic_math.h"

namespace adaisp {
namespace {

constexpr int TW = 128, TH = 32;

// What a method asks of the tile: R, the ring its filter reaches; STRIDE, the LDS row stride in words; border(), the
// reflection that serves that ring.
// Bilinear: 34 x 130 staged, rows two words apart from the staged width (132).
// MHC: 36 x 132 staged, and the row stride is the staged width itself: the staging index IS the LDS address (consecutive
// lanes, consecutive banks), and 132 is even, so a lane's six samples of a row, starting at the even column 2 cx, are
// three aligned 8-byte reads; a wave reads one row at a time (all 64 cell columns of it), 64 consecutive dwords per
// half-wave, so neither the row taps nor the column taps (which are other rows, read by the same lane) meet a bank twice.
template <int METHOD>
struct Tile {
    static constexpr int R = METHOD == ADAISP_DEMOSAIC_MHC ? 2 : 1;
    static constexpr int LW = TW + 2 * R, LH = TH + 2 * R;
    static constexpr int STRIDE = METHOD == ADAISP_DEMOSAIC_MHC ? LW : LW + 2;
    static __device__ __forceinline__ int border(int i, int n) { return R == 2 ? reflect2(i, n) : mirror(i, n); }
};

// The three planes of a pixel pair at (Y, gx) of the frame. Cells are aligned to the frame: 8-byte stores when FW is even
// and `out` 8-byte aligned (VEC), one store per sample otherwise.
template <bool VEC>
__device__ __forceinline__ void store_pair(float* __restrict__ o, long plane, int FW, int Y, int gx, const float (&r)[2],
                                           const float (&g)[2], const float (&bl)[2]) {
    const long off = (long)Y * FW + gx;
    if (VEC) {
        *reinterpret_cast<float2*>(o + off) = make_float2(r[0], r[1]);
        *reinterpret_cast<float2*>(o + plane + off) = make_float2(g[0], g[1]);
        *reinterpret_cast<float2*>(o + 2 * plane + off) = make_float2(bl[0], bl[1]);
    } else {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
            if (gx + dx < FW) {
                o[off + dx] = r[dx];
                o[plane + off + dx] = g[dx];
                o[2 * plane + off + dx] = bl[dx];
            }
    }
}

// RECTS == false: the image is the frame (adaisp_demosaic_ex; FH, FW even, `desc` null and never read, VEC).
// RECTS == true: the same rule inside every image's own rectangle of a letterboxed frame (adaisp_demosaic_rects_ex,
// FH = FW = S): the plane of adaisp_unprocess_bayer holds image b at (top, left), h x w, and black around it. The CFA
// phase and the reflection belong to the rectangle (iy = y - top, ix = x - left), so a border pixel never averages with
// the pad and an odd top / left keeps the colours in place; every output outside the rectangle is exactly 0. As
// adaisp_unprocess_bayer, a placement that does not fit the frame is never read from, and an image without a second row
// or column has nothing to reflect onto: both come out all zero. The tile grid covers the frame; the staging reads
// through the rectangle's reflection (and its clamp), so a tile's ring comes from inside the image whatever lies beside
// it. A tile that misses the rectangle stages nothing and writes zeros; inside a tile that hits, every LDS sample is
// staged, so the filters run on all cells and the rectangle test only selects between their result and 0.
template <int METHOD, bool RECTS, bool VEC>
__global__ __launch_bounds__(256) void k_demosaic(const unsigned short* __restrict__ raw,
                                                  const adaisp_unprocess_desc* __restrict__ desc, float* __restrict__ out,
                                                  int FH, int FW, int ry, int rx, float black, float inv_range) {
    using T = Tile<METHOD>;
    __shared__ __attribute__((aligned(8))) float s[T::LH][T::STRIDE];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    int h = FH, w = FW, top = 0, left = 0;
    bool hit = true;                                                             // workgroup-uniform
    if (RECTS) {
        const adaisp_unprocess_desc& d = desc[b];
        h = d.h, w = d.w, top = d.top, left = d.left;
        const bool fits = h >= 2 && w >= 2 && top >= 0 && left >= 0 && top <= FH - h && left <= FW - w;
        hit = fits && y0 < top + h && y0 + TH > top && x0 < left + w && x0 + TW > left;
    }
    const long plane = (long)FH * FW;
    if (hit) {
        const unsigned short* __restrict__ src = raw + (long)b * plane + (long)top * FW + left;
        for (int i = threadIdx.x; i < T::LH * T::LW; i += 256) {
            const int ly = i / T::LW, lx = i - ly * T::LW;
            const int y = T::border(y0 + ly - T::R - top, h), x = T::border(x0 + lx - T::R - left, w);
            (&s[0][0])[T::STRIDE == T::LW ? i : ly * T::STRIDE + lx] = raw_sample<METHOD>(src[(long)y * FW + x], black, inv_range);
        }
        __syncthreads();
    }
    float* __restrict__ o = out + (long)b * 3 * plane;
    // 64 x 16 cells per tile, 4 per thread: thread -> cell column (tid & 63) and four cell rows of its wave
    const int cx = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx = x0 + 2 * cx;
    // one pixel row of a cell: the sites (Y, gx) and (Y, gx + 1), the first one's neighbourhood through at(dy, dx)
    auto row = [&](int Y, auto at) {
        if (RECTS && Y >= FH) return;                                            // odd FH: the last cell row is half a cell
        float r[2], g[2], bl[2];
        const int iy = Y - top;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int ix = gx + dx - left;
            r[dx] = g[dx] = bl[dx] = 0.0f;
            if (!hit) continue;
            float fr, fg, fb;
            raw_site<METHOD>([&](int ddy, int ddx) { return at(ddy, dx + ddx); }, (iy - ry) & 1, (ix - rx) & 1, inv_range,
                             fr, fg, fb);
            if (!RECTS || (iy >= 0 && iy < h && ix >= 0 && ix < w)) { r[dx] = fr; g[dx] = fg; bl[dx] = fb; }
        }
        store_pair<VEC>(o, plane, FW, Y, gx, r, g, bl);
    };
    if (METHOD == ADAISP_DEMOSAIC_MHC) {
        // cell rows 4 wave + k: they ADJOIN (pixel rows 8 wave .. 8 wave + 7), so their 6-row windows overlap, 12 LDS rows
        // serve what 24 would, and a store is still 512 contiguous bytes per wave and row. One lane's 12 x 6 window: LDS
        // rows 8 wave .. 8 wave + 11, columns 2 cx .. 2 cx + 5; pixel (8 wave + j, 2 cx + i) of the tile is v[j + 2][i + 2].
        if (gx >= FW || y0 + 8 * wave >= FH) return;
        float v[12][6];
        if (hit) {
#pragma unroll
            for (int j = 0; j < 12; ++j)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float2 p = *reinterpret_cast<const float2*>(&s[8 * wave + j][2 * cx + 2 * i]);
                    v[j][2 * i] = p.x;
                    v[j][2 * i + 1] = p.y;
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gy = y0 + 8 * wave + 2 * k;
            if (gy >= FH) break;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
                row(gy + dy, [&](int ddy, int ddx) { return v[2 * k + dy + 2 + ddy][2 + ddx]; });
        }
    } else {
        // cell rows wave + 4k, read straight from LDS
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cy = wave + 4 * k;
            const int gy = y0 + 2 * cy;
            if (gx >= FW || gy >= FH) continue;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int ly = 2 * cy + dy + 1, lx = 2 * cx + 1;
                row(gy + dy, [&](int ddy, int ddx) { return s[ly + ddy][lx + ddx]; });
            }
        }
    }
}

template <int METHOD>
hipError_t launch(const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int FH, int FW, int pattern,
                  float black, float white, hipStream_t s) {
    const int ry = pattern >> 1, rx = pattern & 1;
    const dim3 grid((FW + TW - 1) / TW, (FH + TH - 1) / TH, B);
    const float inv = 1.0f / (white - black);
    if (!desc)
        hipLaunchKernelGGL((k_demosaic<METHOD, false, true>), grid, dim3(256), 0, s, raw, desc, out, FH, FW, ry, rx, black, inv);
    else if (FW % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0)
        hipLaunchKernelGGL((k_demosaic<METHOD, true, true>), grid, dim3(256), 0, s, raw, desc, out, FH, FW, ry, rx, black, inv);
    else
        hipLaunchKernelGGL((k_demosaic<METHOD, true, false>), grid, dim3(256), 0, s, raw, desc, out, FH, FW, ry, rx, black, inv);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_demosaic(int method, const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int FH,
                           int FW, int pattern, float black, float white, hipStream_t s) {
    return method == ADAISP_DEMOSAIC_MHC ? launch<ADAISP_DEMOSAIC_MHC>(raw, desc, out, B, FH, FW, pattern, black, white, s)
                                         : launch<ADAISP_DEMOSAIC_BILINEAR>(raw, desc, out, B, FH, FW, pattern, black, white, s);
}

}  // namespace adaisp
