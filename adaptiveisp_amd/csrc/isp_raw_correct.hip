// Raw-capture correction (include/adaisp.h, adaisp_raw_correct): packed native-size uint16 colour-filter-array planes ->
// corrected uint16 planes of the same sizes in ONE launch: defect pixels clamped to their same-position neighbours,
// lens-shading gain from a per-position grid, per-position black level and scale, a new pedestal. Everything is keyed by the
// position k = 2 * (y & 1) + (x & 1) in the 2 x 2 tile, so the kernel knows no colour-filter pattern. The arithmetic and its
// order are the interface (the header states them; tests/_rawfixref.py restates them in numpy): every fp32 operation below
// is written as one rounding.
//
// Mapping. A workgroup (256 lanes) takes tiles of RF_ROWS x RF_COLS samples of one image (blockIdx.z), grid-stride over the
// image's tiles: the host does not know the sizes (the descriptors live on the device), so an image with fewer tiles than
// the grid has workgroups simply leaves some without work. A tile and, when the defect rule is on, its 2-sample ring are
// staged as uint16 in LDS, the way k_raw_load stages rows: 16-byte loads from the first 16-byte boundary of each row on,
// 2-byte loads at the ragged ends and for the mirrored ring (reflect2: period 2n - 2, which keeps the position). Then a
// lane owns 8 consecutive samples of a row, cut at the 16-byte boundaries of the DESTINATION row (rows of odd width start
// at every alignment): the 8 results leave as one 16-byte store; the chunks that hang over the tile's ends are written
// sample by sample. Without the defect rule no lane needs another lane's samples: nothing is staged, and a lane reads its 8
// samples itself (one 16-byte load where the source chunk is aligned as the destination's is). The plane crosses HBM once
// in each direction.
//
// LDS columns are padded by one word per 8 samples, so the lanes of a row (8 samples = 4 words apart) start 5 words apart
// and their reads spread over the banks.
#include "isp_internal.h"
#include "isp_demosaic_math.h"

#include <stddef.h>

static_assert(sizeof(adaisp_rawfix_desc) == 96, "adaisp_rawfix_desc is 96 bytes (adaptiveisp_amd/_lib.py)");
static_assert(offsetof(adaisp_rawfix_desc, black) == 48 && offsetof(adaisp_rawfix_desc, dpc) == 84, "adaisp_rawfix_desc layout");

namespace adaisp {
namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_ROWS = 16;                          // tile rows
constexpr int RF_COLS = 248;                         // tile columns: 31 chunks of 16 bytes, 32 when the row is not aligned
constexpr int RF_RING = 2;                           // reach of the defect rule
constexpr int RF_LROWS = RF_ROWS + 2 * RF_RING;
constexpr int RF_LCOLS = RF_COLS + 2 * RF_RING;      // staged columns per row, ring included
constexpr int RF_LW = RF_LCOLS + 2 * (RF_LCOLS / 8) + 2;   // LDS samples per row (padded)
constexpr int RF_LOADS = (RF_LCOLS + 6) / 8 + 1;     // most 16-byte chunks a staged row spans, from its boundary on
constexpr int RF_CHUNKS = (RF_COLS + 7 + 7) / 8;     // most 16-byte chunks of a destination row a tile touches
constexpr int RF_MAX_GRID = 2048;                    // workgroups per launch, about (256 CUs x 8)

__device__ __forceinline__ int pad8(int l) { return l + ((l >> 3) << 1); }

__device__ __forceinline__ bool finite4(const float* v) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]);
}

// the four table values around a sample, kept while the lane's next samples of the same position stay in the same cell
struct Cell {
    int ix = -1;
    float t00, t01, t10, t11;
};

__global__ __launch_bounds__(RF_THREADS) void k_raw_correct(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            uint8_t* __restrict__ dst, int64_t dst_bytes,
                                                            const adaisp_rawfix_desc* __restrict__ desc,
                                                            const float* __restrict__ gains, int64_t gain_words) {
    __shared__ uint16_t tile[RF_LROWS][RF_LW];
    __shared__ float par[9];                                                 // black[4], scale[4], black_out
    const int tid = threadIdx.x;
    const adaisp_rawfix_desc* __restrict__ dp = desc + blockIdx.z;
    const int64_t so = dp->src_offset, dof = dp->dst_offset, gofs = dp->grid;
    const int H = dp->src_h, W = dp->src_w, gh = dp->grid_h, gw = dp->grid_w, dpc_in = dp->dpc;
    const float step_y = dp->step_y, step_x = dp->step_x;

    // everything here is workgroup-uniform
    const int64_t bytes = (int64_t)H * W * 2;
    bool ok = H >= 2 && W >= 2 && so >= 0 && !(so & 1) && so <= src_bytes && bytes <= src_bytes - so && dof >= 0 &&
              !(dof & 1) && dof <= dst_bytes && bytes <= dst_bytes - dof;
    const bool shade = gofs >= 0;
    if (shade)
        ok = ok && gains != nullptr && gh >= 2 && gw >= 2 && gofs <= gain_words && (int64_t)4 * gh * gw <= gain_words - gofs;
    ok = ok && finite4(dp->scale);
    if (!ok) return;
    if (tid < 4) par[tid] = dp->black[tid];
    else if (tid < 8) par[tid] = dp->scale[tid - 4];
    else if (tid == 8) par[8] = dp->black_out;

    const bool defect = dpc_in >= 0;
    const int dpc = min(dpc_in, 65536);                                      // beyond 65535 nothing can differ: no overflow
    const int R = defect ? RF_RING : 0;
    const uint16_t* __restrict__ img = reinterpret_cast<const uint16_t*>(src + so);
    uint16_t* __restrict__ o = reinterpret_cast<uint16_t*>(dst + dof);
    const float* __restrict__ T = shade ? gains + gofs : nullptr;
    const int64_t gplane = (int64_t)gh * gw;
    const int tx_n = (W + RF_COLS - 1) / RF_COLS, ty_n = (H + RF_ROWS - 1) / RF_ROWS;
    const int64_t ntiles = (int64_t)tx_n * ty_n;

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int y0 = (int)(t / tx_n) * RF_ROWS, c0 = (int)(t % tx_n) * RF_COLS;
        const int th = min(RF_ROWS, H - y0), tw = min(RF_COLS, W - c0);
        const int org = c0 - RF_RING;                                        // LDS column = source column - org
        const int u0 = max(c0 - R, 0), u1 = min(c0 + tw - 1 + R, W - 1);     // staged straight from the row
        __syncthreads();                                                     // the last tile is no longer read; par is set

        // ---- stage rows y0 - R .. y0 + th - 1 + R: RF_LOADS chunk items and one item for the mirrored ring per row
        // (without the defect rule nothing is shared between lanes: they read their samples themselves, below)
        const int nrows = defect ? th + 2 * R : 0;
        for (int it = tid; it < nrows * (RF_LOADS + 1); it += RF_THREADS) {
            const int rr = it / (RF_LOADS + 1), q = it - rr * (RF_LOADS + 1);
            const int r = y0 - R + rr;
            const uint16_t* __restrict__ row = img + (int64_t)reflect2(r, H) * W;
            uint16_t* __restrict__ ls = tile[r - y0 + RF_RING];
            if (q == RF_LOADS) {                                             // the reflected ring: -2, -1, W, W + 1
                if (R) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int u = e < 2 ? e - 2 : W + e - 2;
                        if (u >= c0 - R && u <= c0 + tw - 1 + R) ls[pad8(u - org)] = row[reflect2(u, W)];
                    }
                }
                continue;
            }
            const int ua = u0 - (int)((reinterpret_cast<uintptr_t>(row + u0) >> 1) & 7);       // 16-byte boundary
            const int ub = ua + 8 * q;
            if (ub > u1) continue;
            if (ub >= u0 && ub + 7 <= u1) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + ub);
                const unsigned p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ls[pad8(ub + 2 * e - org)] = (uint16_t)(p[e] & 0xffffu);
                    ls[pad8(ub + 2 * e + 1 - org)] = (uint16_t)(p[e] >> 16);
                }
            } else {
                for (int e = 0; e < 8; ++e) {
                    const int u = ub + e;
                    if (u >= u0 && u <= u1) ls[pad8(u - org)] = row[u];
                }
            }
        }
        __syncthreads();

        // ---- a lane per 16-byte chunk of a destination row
        for (int it = tid; it < th * RF_CHUNKS; it += RF_THREADS) {
            const int yy = it / RF_CHUNKS, j = it - yy * RF_CHUNKS;
            const int y = y0 + yy;
            uint16_t* __restrict__ drow = o + (int64_t)y * W;
            const int xb = c0 - (int)((reinterpret_cast<uintptr_t>(drow + c0) >> 1) & 7) + 8 * j;
            if (xb >= c0 + tw) continue;
            const uint16_t* __restrict__ lc = tile[yy + RF_RING];
            const uint16_t* __restrict__ lu = tile[yy];
            const uint16_t* __restrict__ ld = tile[yy + 2 * RF_RING];

            // the shading row: the same for the lane's 8 samples
            int iy = 0;
            float wy = 0.0f;
            if (shade) {
                const float fy = __fmul_rn((float)y, step_y);
                iy = min((int)fminf(fmaxf(fy, 0.0f), 2147483520.0f), gh - 2);   // min((int)fy, gh - 2), total
                wy = __fsub_rn(fy, (float)iy);
            }
            Cell cell[2];
            const int kr = 2 * (y & 1);
            const float black_out = par[8];
            const bool whole = xb >= c0 && xb + 7 < c0 + tw;
            unsigned own[8] = {0, 0, 0, 0, 0, 0, 0, 0};                       // the lane's samples when there is no LDS tile
            if (!defect) {
                const uint16_t* __restrict__ srow = img + (int64_t)y * W;
                if (whole && !(reinterpret_cast<uintptr_t>(srow + xb) & 15)) {
                    const uint4 v = *reinterpret_cast<const uint4*>(srow + xb);
                    const unsigned p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        own[2 * e] = p[e] & 0xffffu;
                        own[2 * e + 1] = p[e] >> 16;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (xb + e >= c0 && xb + e < c0 + tw) own[e] = srow[xb + e];
                }
            }

            auto one = [&](int e) -> unsigned {
                const int x = xb + e, l = x - org, k = kr + (x & 1);
                int v = (int)own[e];
                if (defect) {
                    v = lc[pad8(l)];
                    const int a0 = lu[pad8(l - 2)], a1 = lu[pad8(l)], a2 = lu[pad8(l + 2)];
                    const int a3 = lc[pad8(l - 2)], a4 = lc[pad8(l + 2)];
                    const int a5 = ld[pad8(l - 2)], a6 = ld[pad8(l)], a7 = ld[pad8(l + 2)];
                    const int hi = max(max(max(a0, a1), max(a2, a3)), max(max(a4, a5), max(a6, a7)));
                    const int lo = min(min(min(a0, a1), min(a2, a3)), min(min(a4, a5), min(a6, a7)));
                    if (v > hi + dpc) v = hi;
                    else if (v + dpc < lo) v = lo;
                }
                float g = 1.0f;
                if (shade) {
                    const float fx = __fmul_rn((float)x, step_x);
                    const int ix = min((int)fminf(fmaxf(fx, 0.0f), 2147483520.0f), gw - 2);
                    const float wx = __fsub_rn(fx, (float)ix);
                    Cell& c = cell[e & 1];                                   // e & 1 <-> one parity of x <-> one position
                    if (c.ix != ix) {
                        const float* __restrict__ tp = T + k * gplane + (int64_t)iy * gw + ix;
                        c.ix = ix;
                        c.t00 = tp[0];
                        c.t01 = tp[1];
                        c.t10 = tp[gw];
                        c.t11 = tp[gw + 1];
                    }
                    const float a = __fadd_rn(c.t00, __fmul_rn(wx, __fsub_rn(c.t01, c.t00)));
                    const float b = __fadd_rn(c.t10, __fmul_rn(wx, __fsub_rn(c.t11, c.t10)));
                    g = __fadd_rn(a, __fmul_rn(wy, __fsub_rn(b, a)));
                }
                float u = __fmul_rn(__fsub_rn((float)v, par[k]), g);
                u = __fadd_rn(__fmul_rn(u, par[4 + k]), black_out);
                return (unsigned)fminf(fmaxf(rintf(u), 0.0f), 65535.0f);     // fmaxf(NaN, 0) = 0
            };

            if (whole) {
                unsigned r[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) r[e] = one(e);
                *reinterpret_cast<uint4*>(drow + xb) =
                    make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (xb + e >= c0 && xb + e < c0 + tw) drow[xb + e] = (uint16_t)one(e);
            }
        }
    }
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_raw_correct(const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes,
                                  const adaisp_rawfix_desc* desc, const float* gains, size_t gain_words, int B,
                                  void* stream) {
    using namespace adaisp;
    if (!src || !dst || !desc || (!gains && gain_words > 0) || B < 0) return ADAISP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 1) return ADAISP_EINVAL;   // uint16 samples
    if (src_bytes > (size_t)INT64_MAX || dst_bytes > (size_t)INT64_MAX || gain_words > (size_t)INT64_MAX) return ADAISP_EINVAL;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return ADAISP_EALIAS;                 // the defect rule reads neighbours
    if (B > 65535) return ADAISP_ESHAPE;                                                  // grid.z
    if (B == 0) return ADAISP_OK;
    const int gx = RF_MAX_GRID / B > 0 ? RF_MAX_GRID / B : 1;
    hipLaunchKernelGGL(k_raw_correct, dim3((unsigned)gx, 1, (unsigned)B), dim3(RF_THREADS), 0,
                       static_cast<hipStream_t>(stream), src, (int64_t)src_bytes, dst, (int64_t)dst_bytes, desc, gains,
                       (int64_t)gain_words);
    return hipGetLastError() == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
