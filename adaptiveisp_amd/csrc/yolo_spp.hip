// Spatial pyramid pooling (yolov3/models/common.py:202-215: SPP(k = (5, 9, 13))): the three stride-1 max pools of one map in
// ONE launch, and their gradient in one launch. NHWC bf16 with channel strides; a lane owns 8 channels (16 bytes) of one pixel.
// gfx950 only.
//
// Forward. With windows clipped at the border (= MaxPool2d's -inf padding) mp9 = mp5 o mp5 and mp13 = mp5 o mp5 o mp5 hold
// exactly, and a max over a square is a max over rows of maxima over columns: a workgroup stages a 16 x 16 tile with a 6-pixel
// halo in LDS (out-of-image pixels as -inf) and runs three cascaded separable 5-pools on it, 8 compares per element and pool
// instead of 25 / 81 / 169. bf16 values are kept as int16 that order like the numbers (sortable2), so one v_pk_max_i16 takes the
// max of two channels.
//
// Backward. grad_x[p] (=|+=) sum_k sum_q [argmax_k(q) == p] grad_out_k[q], argmax_k(q) = the FIRST maximum of q's clipped window
// in row-major order (strict >: how torch's max_pool2d routes its gradient). No atomics: a workgroup owns a 16 x 16 tile of p and
// GATHERS. It recomputes the argmax of every q within 6 pixels of its tile from x (a 12-pixel halo of x in LDS) — separably too:
// the first maximum in row-major order lies in the first row whose row maximum is the window's maximum, at the first column of
// that row that reaches it, so a max over keys (value << 16 | 15 - dy << 4 | 15 - dx) of row keys (value << 16 | 15 - dx) finds
// it in 2 k compares. The gather is separable the same way: every q of one column whose argmax lies in row r sends its gradient
// to the SAME pixel of that row (the one the row key of (r, column) names), so p's row first sums, per q column, grad_out_k[q]
// (staged in LDS) over the k candidates q whose argmax row it is, and p then adds the sums of the k columns whose row key
// names p: 2 k compare-and-adds per pool instead of k x k. Fixed order, fp32 sums, one rounding to bf16: the same bits on every
// run.
#include "yolo_device.h"

namespace adayolo {
namespace {

typedef __attribute__((ext_vector_type(2))) short s16x2;

// ---- forward --------------------------------------------------------------------------------------------------------------
constexpr int F_T = 16, F_L = F_T + 12, F_CG = 2;         // tile edge, tile + halo, 8-channel groups per workgroup
constexpr unsigned kNegInf2 = 0x807F807Fu;                // sortable2(bf16 -inf pair)

// a bf16 pair <-> a pair of int16 that compare like the numbers (negative values: the magnitude bits flipped). Its own inverse.
__device__ __forceinline__ unsigned sortable2(unsigned v) { return v ^ (((v >> 15) & 0x00010001u) * 0x7FFFu); }
__device__ __forceinline__ u32x4 sortable8(u32x4 v) {
    return u32x4{sortable2(v[0]), sortable2(v[1]), sortable2(v[2]), sortable2(v[3])};
}
__device__ __forceinline__ unsigned max2(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ u32x4 max8(u32x4 a, u32x4 b) {
    return u32x4{max2(a[0], b[0]), max2(a[1], b[1]), max2(a[2], b[2]), max2(a[3], b[3])};
}

// One 5 x 5 pool of the LDS tile `a`, whose rows and columns [M, F_L - M) are valid, through `b`; valid afterwards:
// [M + 2, F_L - M - 2). Ends behind a barrier.
template <int M>
__device__ __forceinline__ void pool5(u32x4* a, u32x4* b, int tid) {
    constexpr int R = F_L - 2 * M, Wc = R - 4;
    for (int i = tid; i < R * Wc * F_CG; i += 256) {          // rows: b = max over 5 columns of a
        const int cg = i % F_CG, p = i / F_CG, x = p % Wc + M + 2, y = p / Wc + M;
        const int at = (y * F_L + x) * F_CG + cg;
        u32x4 m = max8(a[at - 2 * F_CG], a[at - F_CG]);
        m = max8(m, a[at]);
        m = max8(m, a[at + F_CG]);
        b[at] = max8(m, a[at + 2 * F_CG]);
    }
    __syncthreads();
    for (int i = tid; i < Wc * Wc * F_CG; i += 256) {         // columns: a = max over 5 rows of b
        const int cg = i % F_CG, p = i / F_CG, x = p % Wc + M + 2, y = p / Wc + M + 2;
        const int at = (y * F_L + x) * F_CG + cg;
        u32x4 m = max8(b[at - 2 * F_L * F_CG], b[at - F_L * F_CG]);
        m = max8(m, b[at]);
        m = max8(m, b[at + F_L * F_CG]);
        a[at] = max8(m, b[at + 2 * F_L * F_CG]);
    }
    __syncthreads();
}

// (no __restrict__: in the engine x and out are channel slices of one buffer — disjoint bytes, one allocation)
__global__ __launch_bounds__(256) void k_spp_fwd(const unsigned short* x, int x_cs, unsigned short* out, int out_cs, int H, int W,
                                                 int C, int tiles_x, int tiles_y) {
    __shared__ u32x4 sa[F_L * F_L * F_CG], sb[F_L * F_L * F_CG];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int cg0 = blockIdx.y * F_CG, ncg = C / 8;
    const int y0 = ty * F_T, x0 = tx * F_T;
    const long img = (long)b * H * W;
    for (int i = tid; i < F_L * F_L * F_CG; i += 256) {
        const int cg = i % F_CG, p = i / F_CG, lx = p % F_L, ly = p / F_L;
        const int gy = y0 - 6 + ly, gx = x0 - 6 + lx;
        u32x4 v = {kNegInf2, kNegInf2, kNegInf2, kNegInf2};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W && cg0 + cg < ncg)
            v = sortable8(*reinterpret_cast<const u32x4*>(x + (img + (long)gy * W + gx) * x_cs + (cg0 + cg) * 8));
        sa[i] = v;
    }
    __syncthreads();
    auto store = [&](int k) {                                 // the tile's own pixels of `sa` -> channel slice k of out
        for (int i = tid; i < F_T * F_T * F_CG; i += 256) {
            const int cg = i % F_CG, p = i / F_CG, lx = p % F_T, ly = p / F_T;
            const int gy = y0 + ly, gx = x0 + lx;
            if (gy < H && gx < W && cg0 + cg < ncg)
                *reinterpret_cast<u32x4*>(out + (img + (long)gy * W + gx) * out_cs + (long)k * C + (cg0 + cg) * 8) =
                    sortable8(sa[((ly + 6) * F_L + lx + 6) * F_CG + cg]);
        }
    };
    // (a store reads sa; the next pool5 overwrites sa only behind its first barrier)
    pool5<0>(sa, sb, tid);
    store(0);
    pool5<2>(sa, sb, tid);
    store(1);
    pool5<4>(sa, sb, tid);
    store(2);
}

// ---- backward -------------------------------------------------------------------------------------------------------------
constexpr int B_T = 16, B_Q = B_T + 12, B_X = B_T + 24;   // tile of p, the q that can name a p of it, the x their windows read
constexpr int kSppBwdLds = B_X * B_X * 16 + B_X * B_Q * 32 + B_Q * B_Q * 8 + B_Q * B_Q * 16;

// bf16 bits -> uint16 that orders like the number, -0 == +0 (torch's > does not tell them apart); 0 is below every value
__device__ __forceinline__ unsigned ukey(unsigned h) {
    h = h == 0x8000u ? 0u : h;
    return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
__device__ __forceinline__ unsigned ukey2(unsigned v) { return ukey(v & 0xFFFFu) | (ukey(v >> 16) << 16); }

// One pool size (window 2 * HW + 1) of the backward: ends with every thread's acc updated and behind a barrier.
template <int HW>
__device__ __forceinline__ void spp_bwd_pool(const u32x4* xs, u32x4* rk, u32x2* am, u32x4* go, const unsigned short* gk, int go_cs,
                                             long img, int H, int W, int y0, int x0, int tid, float (&acc)[8]) {
    constexpr int K = 2 * HW + 1, RR = B_Q + 2 * HW;
    // this pool's slice of grad_out over the q region (zeros outside the image)
    for (int i = tid; i < B_Q * B_Q; i += 256) {
        const int qy = i / B_Q, qx = i % B_Q, gy = y0 - 6 + qy, gx = x0 - 6 + qx;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const u32x4*>(gk + (img + (long)gy * W + gx) * go_cs);
        go[i] = v;
    }
    // row keys: for every x row a window of the q region reads and every q column, the maximum of the K columns around it and
    // the first column offset that reaches it
    for (int i = tid; i < RR * B_Q; i += 256) {
        const int ry = i / B_Q + 6 - HW, qx = i % B_Q;
        const u32x4* s = xs + ry * B_X + qx + 6 - HW;
        unsigned m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const u32x4 v = s[dx];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[2 * j] = max(m[2 * j], (v[j] << 16) | (unsigned)(15 - dx));
                m[2 * j + 1] = max(m[2 * j + 1], (v[j] & 0xFFFF0000u) | (unsigned)(15 - dx));
            }
        }
        rk[2 * (ry * B_Q + qx)] = u32x4{m[0], m[1], m[2], m[3]};
        rk[2 * (ry * B_Q + qx) + 1] = u32x4{m[4], m[5], m[6], m[7]};
    }
    __syncthreads();
    // argmax of every q as a byte per channel: dy << 4 | dx, offsets from the window's first row / column; 0xFF outside the image
    // (the gather reads dy; dx is the row key's)
    for (int i = tid; i < B_Q * B_Q; i += 256) {
        const int qy = i / B_Q, qx = i % B_Q, gy = y0 - 6 + qy, gx = x0 - 6 + qx;
        u32x2 code = {0xFFFFFFFFu, 0xFFFFFFFFu};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            unsigned m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
                const u32x4* s = rk + 2 * ((qy + 6 - HW + dy) * B_Q + qx);
                const u32x4 lo = s[0], hi = s[1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m[j] = max(m[j], lo[j] | (unsigned)((15 - dy) << 4));
                    m[4 + j] = max(m[4 + j], hi[j] | (unsigned)((15 - dy) << 4));
                }
            }
            code = u32x2{0u, 0u};
#pragma unroll
            for (int j = 0; j < 8; ++j) code[j >> 2] |= (0xFFu ^ (m[j] & 0xFFu)) << (8 * (j & 3));
        }
        am[i] = code;
    }
    __syncthreads();
    // gather, rows: T[i][qx] = the sum of go over the q of column qx whose argmax lies in row i of the tile (ascending q row).
    // T row i takes an rk row the column pass is done with and the next step does not read (those are the tile's own 16)
    auto trow = [](int i) { return i < 12 ? i : i + 16; };
    for (int it = tid; it < B_T * B_Q; it += 256) {
        const int i = it / B_Q, qx = it % B_Q;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int dy = -HW; dy <= HW; ++dy) {
            const int qi = (i + 6 + dy) * B_Q + qx;
            const u32x2 a = am[qi];
            const u32x4 g = go[qi];
            const unsigned want = (unsigned)(HW - dy);                            // q's argmax row is row i
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned row = (a[j >> 2] >> (8 * (j & 3) + 4)) & 0xFu;
                const float gv = (j & 1) ? hi_f(g[j >> 1]) : lo_f(g[j >> 1]);
                s[j] += row == want ? gv : 0.0f;
            }
        }
        f32x4* t = reinterpret_cast<f32x4*>(rk + 2 * (trow(i) * B_Q + qx));
        t[0] = f32x4{s[0], s[1], s[2], s[3]};
        t[1] = f32x4{s[4], s[5], s[6], s[7]};
    }
    __syncthreads();
    // gather, columns: thread = one p of the tile; the q columns whose key of p's row names p's column (ascending column)
    const int py = tid / B_T, px = tid % B_T;
#pragma unroll 1
    for (int dx = -HW; dx <= HW; ++dx) {
        const int qx = px + 6 + dx;
        const u32x4* key = rk + 2 * ((py + 12) * B_Q + qx);
        const f32x4* t = reinterpret_cast<const f32x4*>(rk + 2 * (trow(py) * B_Q + qx));
        const u32x4 lo = key[0], hi = key[1];
        const f32x4 t0 = t[0], t1 = t[1];
        const unsigned want = 15u - (unsigned)(HW - dx);                          // the key holds 15 - (column offset in its window)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] += (lo[j] & 0xFu) == want ? t0[j] : 0.0f;
            acc[4 + j] += (hi[j] & 0xFu) == want ? t1[j] : 0.0f;
        }
    }
    __syncthreads();                                          // the next pool restages go / rk / am
}

__global__ __launch_bounds__(256) void k_spp_bwd(const unsigned short* x, int x_cs, const unsigned short* gout, int go_cs,
                                                 unsigned short* gx_, int gx_cs, int accumulate, int H, int W, int C, int tiles_x,
                                                 int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                                   // [B_X][B_X]     8 keys of 16 bits
    u32x4* rk = xs + B_X * B_X;                                                   // [B_X][B_Q][2]  8 keys of 32 bits
    u32x4* go = rk + 2 * B_X * B_Q;                                               // [B_Q][B_Q]     8 bf16
    u32x2* am = reinterpret_cast<u32x2*>(go + B_Q * B_Q);                         // [B_Q][B_Q]     8 bytes
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int ch = blockIdx.y * 8;
    const int y0 = ty * B_T, x0 = tx * B_T;
    const long img = (long)b * H * W;
    for (int i = tid; i < B_X * B_X; i += 256) {
        const int ly = i / B_X, lx = i % B_X, gy = y0 - 12 + ly, gx = x0 - 12 + lx;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            v = *reinterpret_cast<const u32x4*>(x + (img + (long)gy * W + gx) * x_cs + ch);
            v = u32x4{ukey2(v[0]), ukey2(v[1]), ukey2(v[2]), ukey2(v[3])};
        }
        xs[i] = v;
    }
    __syncthreads();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    spp_bwd_pool<2>(xs, rk, am, go, gout + ch, go_cs, img, H, W, y0, x0, tid, acc);
    spp_bwd_pool<4>(xs, rk, am, go, gout + C + ch, go_cs, img, H, W, y0, x0, tid, acc);
    spp_bwd_pool<6>(xs, rk, am, go, gout + 2L * C + ch, go_cs, img, H, W, y0, x0, tid, acc);
    const int gy = y0 + tid / B_T, gx = x0 + tid % B_T;
    if (gy < H && gx < W) {
        u32x4* dst = reinterpret_cast<u32x4*>(gx_ + (img + (long)gy * W + gx) * gx_cs + ch);
        if (accumulate) {
            const u32x4 old = *dst;
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[2 * j] += lo_f(old[j]); acc[2 * j + 1] += hi_f(old[j]); }
        }
        *dst = u32x4{pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7])};
    }
}

}  // namespace

hipError_t launch_spp_fwd(const void* x, int x_cs, void* out, int out_cs, int B, int H, int W, int C, hipStream_t s) {
    const int tiles_x = (W + F_T - 1) / F_T, tiles_y = (H + F_T - 1) / F_T;
    const long blocks = (long)tiles_x * tiles_y * B, groups = (C / 8 + F_CG - 1) / F_CG;
    if (blocks > 0x7fffffffL || groups > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spp_fwd, dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0, s, static_cast<const unsigned short*>(x),
                       x_cs, static_cast<unsigned short*>(out), out_cs, H, W, C, tiles_x, tiles_y);
    return hipGetLastError();
}

hipError_t launch_spp_bwd(const void* x, int x_cs, const void* gout, int go_cs, void* gx, int gx_cs, int accumulate, int B, int H,
                          int W, int C, hipStream_t s) {
    const int tiles_x = (W + B_T - 1) / B_T, tiles_y = (H + B_T - 1) / B_T;
    const long blocks = (long)tiles_x * tiles_y * B;
    if (blocks > 0x7fffffffL || C / 8 > 65535) return hipErrorInvalidValue;
    return launch_lds<k_spp_bwd>(dim3((unsigned)blocks, (unsigned)(C / 8)), dim3(256), kSppBwdLds, s,
                                 static_cast<const unsigned short*>(x), x_cs, static_cast<const unsigned short*>(gout), go_cs,
                                 static_cast<unsigned short*>(gx), gx_cs, accumulate, H, W, C, tiles_x, tiles_y);
}

}  // namespace adayolo
