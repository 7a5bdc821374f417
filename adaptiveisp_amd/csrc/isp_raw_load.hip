// Raw-capture loader (include/adaisp.h, adaisp_raw_load): packed native-size uint16 colour-filter-array planes -> the
// letterboxed [B,3,S,S] fp32 batch in ONE launch: demosaic (the per-site math of isp_demosaic_math.h, so D is bit for bit
// adaisp_demosaic_rects_ex of the whole plane), per-channel gain, separable resample through the host's CSR taps
// (adaptiveisp_amd/resize.py: horizontal pass, then vertical pass, each one fp32 multiply then one fp32 add in tap order
// from 0.0f, adaisp_resize_u8's AREA arithmetic) and placement. The plane is read once, 2 B per native pixel; the
// full-resolution colour image never exists in memory.
//
// Mapping from the output side. A workgroup (128 lanes) owns RL_ROWS consecutive rows of the frame of one image and walks
// the image's columns in groups of G <= 128 output columns, a lane per column. For an output row it walks the row's
// vertical taps; for each tap's source row j it keeps the raw rows j - 2 .. j + 2 in LDS, as fp32 samples already
// converted the way the demosaic wants them, in a rolling window of 5 row slots (slot = row mod 5): going from j to j + 1
// stages one new row, and the window carries on from one output row of the band to the next. Rows are staged
// cooperatively: the group's source span (its first to its last tap, plus the 2-pixel ring, at most RL_CW columns, which
// bounds G: LDS use does not depend on the shrink factor) as 16-byte loads from the first 16-byte boundary of the row on,
// 2-byte loads for the ragged ends and for the reflected ring columns. Neighbouring lanes read columns a shrink factor
// apart, so the LDS column is swizzled (one pad word per 32): strides of 2, 4, 8, 16 land in distinct banks.
// Then every lane runs its own horizontal taps on that row: the 3 x 3 / 5 x 5 neighbourhood from LDS, the site's three
// colours, gain, multiply-add into t; after the taps, acc += wy * t.
//
// Whatever the taps say is computed as specified: a tap whose column lies outside the staged span (a table that is not
// the host's, or a group whose span outgrows RL_CW) takes its neighbourhood from global memory through the same math.
#include "isp_internal.h"
#include "isp_csr.h"
#include "isp_demosaic_math.h"

static_assert(sizeof(adaisp_raw_desc) == 64, "adaisp_raw_desc is 64 bytes (adaptiveisp_amd/_lib.py)");

namespace adaisp {
namespace {

constexpr int RL_THREADS = 128;                 // lanes per workgroup = most output columns per group
constexpr int RL_ROWS = 4;                      // frame rows per workgroup
constexpr int RL_CW = 1280;                     // staged columns per raw row, ring included
constexpr int RL_LW = RL_CW + RL_CW / 32;       // LDS words per row slot (swizzled)
constexpr int RL_WIN = 5;                       // row slots

__device__ __forceinline__ int swz(int l) { return l + (l >> 5); }

// raw_sample<METHOD>() and raw_site<METHOD>(): isp_demosaic_math.h

template <int METHOD>
__global__ __launch_bounds__(RL_THREADS) void k_raw_load(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                         const adaisp_raw_desc* __restrict__ desc,
                                                         const int32_t* __restrict__ tabs, int64_t tab_words,
                                                         float* __restrict__ out, int S, int ry, int rx, float black,
                                                         float inv_range) {
    __shared__ float win[RL_WIN][RL_LW];
    constexpr int R = METHOD == ADAISP_DEMOSAIC_MHC ? 2 : 1;      // rows the filter reaches above and below
    const int tid = threadIdx.x, Y0 = blockIdx.y * RL_ROWS, Y1 = min(Y0 + RL_ROWS, S);
    const adaisp_raw_desc d = desc[blockIdx.z];
    const int H = d.src_h, W = d.src_w, h = d.h, w = d.w, top = d.top, left = d.left;
    const int64_t plane = (int64_t)S * S;
    float* __restrict__ o = out + (int64_t)blockIdx.z * 3 * plane;

    // everything below is workgroup-uniform
    bool ok = H >= 2 && W >= 2 && h >= 1 && w >= 1 && top >= 0 && left >= 0 && top <= S - h && left <= S - w &&
              d.src_offset >= 0 && !(d.src_offset & 1) && d.src_offset <= src_bytes &&
              (int64_t)H * W * 2 <= src_bytes - d.src_offset;
    ok = ok && csr_fits(tabs, d.tab_x, w, tab_words) && csr_fits(tabs, d.tab_y, h, tab_words);

    // the frame around the image (all of it for an image that is not loaded): exactly 0
    for (int Y = Y0; Y < Y1; ++Y) {
        const bool inside = ok && Y >= top && Y < top + h;
        for (int X = blockIdx.x * RL_THREADS + tid; X < S; X += gridDim.x * RL_THREADS)
            if (!inside || X < left || X >= left + w) {
                const int64_t at = (int64_t)Y * S + X;
                o[at] = 0.0f;
                o[plane + at] = 0.0f;
                o[2 * plane + at] = 0.0f;
            }
    }
    if (!ok) return;
    const int y_lo = max(Y0, top) - top, y_hi = min(Y1, top + h) - top;
    if (y_lo >= y_hi) return;

    const uint16_t* __restrict__ img = reinterpret_cast<const uint16_t*>(src + d.src_offset);
    const int32_t* __restrict__ tx = tabs + d.tab_x;
    const int32_t* __restrict__ ty = tabs + d.tab_y;
    // columns per group: the span of G columns shrunk by W / w is under G * W / w + 2; spread evenly, and over the grid
    const int gmax = (int)min<int64_t>(max<int64_t>((int64_t)(RL_CW - 8) * w / W, 1), RL_THREADS);
    const int ng = max((w + gmax - 1) / gmax, min((int)gridDim.x, (w + 63) / 64));
    const int G = (w + ng - 1) / ng;

    for (int grp = blockIdx.x; grp < ng; grp += gridDim.x) {
        const int x0 = grp * G, gw = min(G, w - x0);
        if (gw <= 0) break;
        const bool active = tid < gw;
        const Csr cx = csr_row(tx, w, active ? x0 + tid : x0);
        // staged span: columns cs .. ce have their whole neighbourhood in LDS (LDS column = source column - (cs - 2))
        const Csr cfirst = csr_row(tx, w, x0), clast = csr_row(tx, w, x0 + gw - 1);
        const int cs = cfirst.hi > cfirst.lo ? clampi(cfirst.idx[cfirst.lo], 0, W - 1) : 0;
        int ce = clast.hi > clast.lo ? clampi(clast.idx[clast.hi - 1], 0, W - 1) : cs;
        ce = max(min(ce, cs + RL_CW - 5), cs);
        const int org = cs - 2, u0 = max(org, 0), u1 = min(ce + 2, W - 1);   // u0 .. u1: staged straight from the row
        int have_lo = 1, have_hi = 0;                                        // source rows (unreflected) in the window

        for (int y = y_lo; y < y_hi; ++y) {
            const Csr cy = csr_row(ty, h, y);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (int k = cy.lo; k < cy.hi; ++k) {
                const int j = clampi(cy.idx[k], 0, H - 1);
                const float wy = cy.wt[k];
                if (j - R < have_lo || j + R > have_hi) {
                    __syncthreads();                                         // the rows being replaced are no longer read
                    for (int r = j - R; r <= j + R; ++r) {
                        if (r >= have_lo && r <= have_hi) continue;
                        const uint16_t* __restrict__ row = img + (int64_t)reflect2(r, H) * W;
                        float* __restrict__ ws = win[(r + 2 * RL_WIN) % RL_WIN];
                        const int ua = u0 - (int)((reinterpret_cast<uintptr_t>(row + u0) >> 1) & 7);   // 16-byte boundary
                        const int nchunk = (u1 - ua) / 8 + 1;
                        for (int q = tid; q < nchunk; q += RL_THREADS) {
                            const int ub = ua + 8 * q;
                            if (ub >= u0 && ub + 7 <= u1) {
                                const uint4 v = *reinterpret_cast<const uint4*>(row + ub);
                                const unsigned p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    ws[swz(ub + 2 * e - org)] = raw_sample<METHOD>(p[e] & 0xffffu, black, inv_range);
                                    ws[swz(ub + 2 * e + 1 - org)] = raw_sample<METHOD>(p[e] >> 16, black, inv_range);
                                }
                            } else {
                                for (int e = 0; e < 8; ++e) {
                                    const int u = ub + e;
                                    if (u >= u0 && u <= u1) ws[swz(u - org)] = raw_sample<METHOD>(row[u], black, inv_range);
                                }
                            }
                        }
                        if (tid < 4) {                                       // the reflected ring: -2, -1, W, W + 1
                            const int u = tid < 2 ? tid - 2 : W + tid - 2;
                            if (u >= org && u <= ce + 2)
                                ws[swz(u - org)] = raw_sample<METHOD>(row[reflect2(u, W)], black, inv_range);
                        }
                    }
                    have_lo = j - R;
                    have_hi = j + R;
                    __syncthreads();
                }
                if (!active) continue;
                const float* __restrict__ rows[5];
#pragma unroll
                for (int dy = -2; dy <= 2; ++dy) rows[dy + 2] = win[(j + dy + 2 * RL_WIN) % RL_WIN];
                const int py = (j - ry) & 1;
                float t[3] = {0.0f, 0.0f, 0.0f};
                for (int m = cx.lo; m < cx.hi; ++m) {
                    const int i = clampi(cx.idx[m], 0, W - 1);
                    const float wx = cx.wt[m];
                    const int px = (i - rx) & 1;
                    float v[3];
                    if (i >= cs && i <= ce) {
                        const int l = i - org;
                        raw_site<METHOD>([&](int dy, int dx) { return rows[dy + 2][swz(l + dx)]; }, py, px, inv_range, v[0],
                                         v[1], v[2]);
                    } else {
                        raw_site<METHOD>(
                            [&](int dy, int dx) {
                                return raw_sample<METHOD>(img[(int64_t)reflect2(j + dy, H) * W + reflect2(i + dx, W)], black,
                                                          inv_range);
                            },
                            py, px, inv_range, v[0], v[1], v[2]);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[c] = __fadd_rn(t[c], __fmul_rn(wx, __fmul_rn(v[c], d.gain[c])));
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(wy, t[c]));
            }
            if (active) {
                const int64_t at = (int64_t)(top + y) * S + left + x0 + tid;
                o[at] = acc[0];
                o[plane + at] = acc[1];
                o[2 * plane + at] = acc[2];
            }
        }
        __syncthreads();                                                     // the next group restages every slot
    }
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_raw_load(const uint8_t* src, size_t src_bytes, const adaisp_raw_desc* desc, const int32_t* tabs,
                               size_t tab_words, float* out, int B, int S, int pattern, int method, float black_level,
                               float white_level, void* stream) {
    using namespace adaisp;
    if (!src || !desc || !tabs || !out || B < 0 || S < 1) return ADAISP_EINVAL;
    if (reinterpret_cast<uintptr_t>(src) & 1) return ADAISP_EINVAL;                      // uint16 samples
    if (pattern < 0 || pattern > 3 || !(white_level > black_level)) return ADAISP_EINVAL;
    if (method != ADAISP_DEMOSAIC_BILINEAR && method != ADAISP_DEMOSAIC_MHC) return ADAISP_EINVAL;
    if (src_bytes > (size_t)INT64_MAX || tab_words > (size_t)INT64_MAX) return ADAISP_EINVAL;
    if (B > 65535 || S > 32768) return ADAISP_ESHAPE;                                     // grid.z; 32-bit pixel indices
    if (B == 0) return ADAISP_OK;
    const dim3 grid((unsigned)((S + RL_THREADS - 1) / RL_THREADS), (unsigned)((S + RL_ROWS - 1) / RL_ROWS), (unsigned)B);
    const int ry = pattern >> 1, rx = pattern & 1;
    const float inv = 1.0f / (white_level - black_level);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (method == ADAISP_DEMOSAIC_MHC)
        hipLaunchKernelGGL((k_raw_load<ADAISP_DEMOSAIC_MHC>), grid, dim3(RL_THREADS), 0, s, src, (int64_t)src_bytes, desc, tabs,
                           (int64_t)tab_words, out, S, ry, rx, black_level, inv);
    else
        hipLaunchKernelGGL((k_raw_load<ADAISP_DEMOSAIC_BILINEAR>), grid, dim3(RL_THREADS), 0, s, src, (int64_t)src_bytes, desc,
                           tabs, (int64_t)tab_words, out, S, ry, rx, black_level, inv);
    return hipGetLastError() == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
